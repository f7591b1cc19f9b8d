"""-m gpu: ``sn_yuv_despot`` (csrc/sn_despot.hip) against its restatement (tests/despot_ref.py), byte for byte and count for count, with no tolerance
anywhere; ``despot_vectors`` against motion_ref.block_motion_ref on the stack and on the reversed stack; and the paths that must agree: a second
call on a used destination, a destination inside a larger buffer, a base at an odd address.

Inputs are RANDOM words with T = 8, so seeds are everywhere and every halo and dilation path is hit.  Shapes (H x W): 37 x 83 at 4:2:0 is odd both
ways (the clamped last row and column, the element-wise paths, chroma samples with fewer than four luma samples); 70 x 150 is 3 x 2 workgroups of
128 x 32 with halos across tile and vector-block borders, at 4:4:4 8 bit and 4:2:0 10 bit; 40 x 96 at 10-bit 4:4:4 holds any 16-bit word; 2 x 3 is
one vector block; 1 x 5 has none and is a copy with counts 0.  Every shape runs once with the vectors of ``despot_vectors`` and once with random
int8 vectors that include -128 and 127: the clamp makes these legal inputs."""
import numpy as np
import pytest
import torch

import despot_ref as DR
import motion_ref as MR
import yuv_ref as R
from shiftnet_amd.io_edges import despot_vectors, despot_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

F420 = R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED)
F444 = R.Fmt(8, R.C444, R.BT601, R.FULL)
F420_10 = R.Fmt(10, R.C420_CENTER, R.BT709, R.FULL)
F444_10 = R.Fmt(10, R.C444, R.BT709, R.LIMITED)
S, T = 5, 8
# fmt, H, W, the largest stored word
CASES = {"37x83 420p8": (F420, 37, 83, 255), "70x150 444p8": (F444, 70, 150, 255), "70x150 420p10": (F420_10, 70, 150, 1023),
         "40x96 444p10 any word": (F444_10, 40, 96, 65535), "2x3 420p8": (F420, 2, 3, 255), "1x5 420p8": (F420, 1, 5, 255)}
RANGES = ((1, 3), (2, 1))                                          # (f0, n)


def words(fmt, H, W, top, seed):
    """uint8 [S, frame_bytes]: random words 0 .. top."""
    n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
    a = np.random.default_rng(seed).integers(0, top + 1, (S, n))
    return a.astype("<u2").view(np.uint8).reshape(S, -1) if fmt.bits == 10 else a.astype(np.uint8)


def random_vectors(H, W, seed):
    """Two int8 [S - 1, nby, nbx, 2] of anything, -128 and 127 among them."""
    nby, nbx = MR.grid(H, W)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        v = rng.integers(-128, 128, (S - 1, nby, nbx, 2)).astype(np.int8)
        if v.size >= 2:
            v.reshape(-1)[:2] = (-128, 127)
        out.append(v)
    return out


_inputs = {}


def inputs(case, kind):
    """(payloads, mv_prev, mv_next) of a case on the host, made once: the vectors of the restatement's matcher, or random ones."""
    if (case, kind) not in _inputs:
        fmt, H, W, top = CASES[case]
        src = words(fmt, H, W, top, seed=H * W)
        mvp, mvn = DR.vectors_ref(src, fmt, H, W) if kind == "matcher" else random_vectors(H, W, seed=H + W)
        _inputs[(case, kind)] = (src, np.ascontiguousarray(mvp), np.ascontiguousarray(mvn))
    return _inputs[(case, kind)]


def on_device(src, fmt, H, W, mvp, mvn, f0, n, K, G, chroma, **kw):
    out, counts = despot_yuv(src, yuv_fmt(*fmt), H, W, mvp, mvn, f0, n, T, K, G, chroma, **kw)
    return out.cpu().numpy(), counts.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ["matcher", "random int8"])
@pytest.mark.parametrize("case", list(CASES))
def test_the_kernel_equals_the_restatement_byte_for_byte_and_count_for_count(case, kind):
    fmt, H, W, _ = CASES[case]
    src, mvp, mvn = inputs(case, kind)
    d = torch.from_numpy(src).cuda()
    if kind == "matcher":                                             # the device's vectors are the restatement's: both directions
        dp, dn = despot_vectors(d, yuv_fmt(*fmt), H, W)
        assert np.array_equal(dn.cpu().numpy(), MR.block_motion_ref(src, fmt, H, W)[0])
        assert np.array_equal(dp.cpu().numpy(), MR.block_motion_ref(src[::-1], fmt, H, W)[0][::-1])
        assert np.array_equal(dp.cpu().numpy(), mvp) and np.array_equal(dn.cpu().numpy(), mvn)
    else:
        dp, dn = torch.from_numpy(mvp).cuda(), torch.from_numpy(mvn).cuda()
    seeds = replaced = 0
    for K in (0, 2, 8):
        for G in (0, 1, 2):
            for chroma in ("follow", "off"):
                for f0, n in RANGES:
                    want, wcounts = DR.despot_ref(src, mvp, mvn, fmt, H, W, f0, n, T, K, G, chroma)
                    got, counts = on_device(d, fmt, H, W, dp, dn, f0, n, K, G, chroma)
                    where = (case, kind, K, G, chroma, f0, n)
                    assert got.shape == want.shape and np.array_equal(got, want), (where, int(np.sum(got != want)))
                    assert np.array_equal(counts, wcounts), (where, counts.tolist(), wcounts.tolist())
                    seeds, replaced = seeds + int(wcounts[:, 0].sum()), replaced + int(wcounts[:, 1].sum())
    assert np.array_equal(d.cpu().numpy(), src)                       # the source is read only
    if H < 2:
        assert seeds == 0 and replaced == 0                           # no vector block: a copy, counts 0
    elif H * W > 100:
        assert seeds > 0 and replaced > seeds                         # random words: the rule is at work in every case


def test_a_second_call_on_a_used_destination_gives_the_same_bytes_and_nothing_outside_the_frames_is_touched():
    case = "70x150 420p10"
    fmt, H, W, _ = CASES[case]
    src, mvp, mvn = inputs(case, "matcher")
    d, dp, dn = (torch.from_numpy(a).cuda() for a in (src, mvp, mvn))
    for f0, n in RANGES:
        want, wcounts = DR.despot_ref(src, mvp, mvn, fmt, H, W, f0, n, T, 2, 1, "follow")
        big = torch.full((n + 2, src.shape[1]), 0xA5, dtype=torch.uint8, device="cuda")      # a frame of guard bytes on either side
        cbig = torch.full((n + 2, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        for _ in range(2):                                            # the second call overwrites what the first left, counts included
            got, counts = on_device(d, fmt, H, W, dp, dn, f0, n, 2, 1, "follow", out=big[1:1 + n], out_counts=cbig[1:1 + n])
            assert np.array_equal(got, want) and np.array_equal(counts, wcounts)
        b, c = big.cpu().numpy(), cbig.cpu().numpy()
        assert np.all(b[0] == 0xA5) and np.all(b[-1] == 0xA5) and np.all(c[0] == 0x5A5A5A5A) and np.all(c[-1] == 0x5A5A5A5A)
        other, _ = on_device(d.flip(0).contiguous(), fmt, H, W, dp, dn, f0, n, 2, 1, "follow", out=big[1:1 + n], out_counts=cbig[1:1 + n])
        assert not np.array_equal(other, want)
        got, counts = on_device(d, fmt, H, W, dp, dn, f0, n, 2, 1, "follow", out=big[1:1 + n], out_counts=cbig[1:1 + n])
        assert np.array_equal(got, want) and np.array_equal(counts, wcounts)


@pytest.mark.parametrize("case", ["37x83 420p8", "70x150 444p8"])
def test_a_moved_base_takes_the_element_wise_path_with_the_same_bytes(case):
    fmt, H, W, _ = CASES[case]
    src, mvp, mvn = inputs(case, "matcher")
    fb = src.shape[1]
    dp, dn = torch.from_numpy(mvp).cuda(), torch.from_numpy(mvn).cuda()
    want, wcounts = DR.despot_ref(src, mvp, mvn, fmt, H, W, 1, 3, T, 2, 1, "follow")
    room = torch.zeros(S * fb + 64, dtype=torch.uint8, device="cuda")
    oroom = torch.full((3 * fb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    for off, ooff in ((1, 0), (3, 5), (0, 7)):                       # odd addresses of the source, of the destination, of both
        moved = room[off:off + S * fb].view(S, fb)
        moved.copy_(torch.from_numpy(src).cuda())
        out = oroom[ooff:ooff + 3 * fb].view(3, fb)
        assert moved.data_ptr() % 2 == off % 2 and out.data_ptr() % 2 == ooff % 2
        got, counts = on_device(moved, fmt, H, W, dp, dn, 1, 3, 2, 1, "follow", out=out)
        assert np.array_equal(got, want) and np.array_equal(counts, wcounts), (off, ooff)
        o = oroom.cpu().numpy()
        assert np.all(o[:ooff] == 0xA5) and np.all(o[ooff + 3 * fb:] == 0xA5)
        oroom.fill_(0xA5)
