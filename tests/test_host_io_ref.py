"""CPU tests of what tests/test_gpu_io_edges.py stands on (tests/io_cases.py): the conditions that keep the GPU test honest, and the refusals of the three
entry points of csrc/sn_io.hip, which are judged on the host before anything is launched.

  * The yardstick of ``sn_ssim_u8`` is ``cli.ssim_calculate``, float32 volumes through scipy.  On every float32 case from 6 x 13 upward it is within
    YARDSTICK_TOL = 1e-5 of the same function in float64 -- half of the 2e-5 contract, so the yardstick cannot use up the bound.  Measured here: at most
    6.1e-6 at 6x13, 1.6e-6 at 9x300, 8.8e-6 at 40x56, 2.5e-6 at 130x127, 4.0e-6 at 150x221.  The same inputs rounded to fp16 / bf16 are printed, not
    asserted: bf16 has one code of resolution near white, and there the float32 yardstick is up to 2.7e-5 (6x13) and 1.3e-5 (larger) from float64.
  * ``TIES`` holds its 16 + 16 values and they are ties; the frames of a T = 3 clip differ in SSE and in SSIM; ``equal`` is SSE 0 and SSIM 1.
  * The pass counts of ``SIZES`` are those of sn_egress_blocks() and sn_ssim_blocks()."""
import itertools

import numpy as np
import pytest
import torch

import io_cases as IO
from shiftnet_amd import cli
from shiftnet_amd import lib as L

BIG = [s for s in IO.SIZES if s.H * s.W > 15]


def _rounded(out: np.ndarray, dt) -> np.ndarray:
    return torch.from_numpy(out.copy()).to(dt).float().numpy()


def test_the_float32_yardstick_is_within_half_the_contract_of_float64_on_every_ssim_case():
    worst = {}
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        for s, T in itertools.product(BIG, IO.TS):
            for c in IO.ssim_contents(s.H, s.W):
                gt, out = IO.clip(c, T, s.H, s.W)
                x = _rounded(out, dt)
                for e in range(T):
                    host = IO.host_image(x[e])
                    d = abs(cli.ssim_calculate(host, gt[e]) - IO.ssim_f64(host, gt[e]))
                    worst[(dt, s.H, s.W, c)] = max(worst.get((dt, s.H, s.W, c), 0.0), d)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        for s in BIG:
            row = {c: worst[(dt, s.H, s.W, c)] for c in IO.SSIM_CONTENTS}
            print(f"{str(dt)[6:]} {s.H}x{s.W}: " + ", ".join(f"{c} {v:.2g}" for c, v in row.items()))
    f32 = max(v for k, v in worst.items() if k[0] == torch.float32)
    print(f"float32: the yardstick's largest distance from float64 {f32:.3g}")
    assert f32 <= IO.YARDSTICK_TOL


def test_ties_holds_16_even_and_16_odd_ties_and_the_edge_values():
    t = IO.TIES
    assert t.dtype == np.float32 and len(t) == 32 + len(IO.EDGE_X)
    v = t[:32] * np.float32(255)
    k = np.floor(v).astype(np.int64)
    assert v.dtype == np.float32 and np.array_equal(v, k + np.float32(0.5))                  # the rounded product IS k + 0.5
    assert (k[:16] % 2 == 0).all() and (k[16:] % 2 == 1).all() and len(set(k.tolist())) == 32
    assert np.array_equal(np.rint(v), np.where(k % 2 == 0, k, k + 1))                        # to even: down at even k, up at odd k
    e = IO.EDGE_X
    assert e[0] == 0.5 and e[0] * np.float32(255) == 127.5
    for dt in (torch.float16, torch.bfloat16):
        assert _rounded(e[:3], dt).tolist() == [0.5, 0.0, 1.0]                               # exact in all three dtypes
    assert (e == 0).sum() == 2 and np.signbit(e[3]) and e[3] == 0
    assert e[4] < 0 < e[5] and e[6] < 1 < e[7] and (e < 0).any() and (e > 1).any()
    # frame 0 of the texture clip carries them all from 6 x 13 upward
    _, out = IO.egress_clip("texture", 1, 6, 13)
    assert np.array_equal(out[0].reshape(-1)[:len(t)].view(np.uint32), t.view(np.uint32))


def test_the_frames_of_a_clip_differ_and_equal_is_equal():
    for s in IO.SIZES:
        for c in IO.ssim_contents(s.H, s.W):
            gt, out = IO.clip(c, 3, s.H, s.W)
            _, _, sse = IO.egress_ref(out, gt)
            ssim = [IO.ssim_f64(IO.host_image(out[e]), gt[e]) for e in range(3)]
            if c == "equal":
                assert (sse == 0).all() and all(abs(v - 1) < 1e-12 for v in ssim), (s, sse, ssim)
                assert abs(cli.ssim_calculate(IO.host_image(out[1]), gt[1]) - 1) < 1e-6
                assert cli.psnr_255(IO.host_image(out[1]), gt[1]) == float("inf")
                continue
            assert len(set(sse.tolist())) == 3 and len(set(ssim)) == 3 and (sse > 0).all(), (s, c, sse, ssim)
            assert not np.array_equal(gt[0], gt[1]) or c != "texture"
        for T in IO.TS:
            gt, out = IO.egress_clip("texture", T, s.H, s.W)
            assert out.min() < 0 and out.max() > 1 or s.H * s.W == 1                         # the clamp matters
            gt, out = IO.egress_clip("equal", T, s.H, s.W)
            _, _, sse = IO.egress_ref(out, gt)
            assert (sse[T // 2] == 0) and (T == 1 or (sse[0] > 0 and sse[2] > 0))             # an equal frame between two that are not


def test_the_pass_counts_of_the_size_table_are_the_librarys():
    lib = L.load()
    eg, ss = lib.sn_egress_blocks() * 256, lib.sn_ssim_blocks() * 256
    for s in IO.SIZES:
        assert (-(-(s.H * s.W) // eg), -(-(s.H * s.W) // ss)) == (s.egress_passes, s.ssim_passes), s
    assert max(s.egress_passes for s in IO.SIZES) >= 3 and max(s.ssim_passes for s in IO.SIZES) >= 2
    assert IO.sse_bound(1.0, 130, 127) == (3 * 2 + 14) * 2.0 ** -24 and IO.sse_bound(1.0, 1, 1, eg) == 17 * 2.0 ** -24
    # 130 x 127: the second pass is for 126 pixels, all of workgroup 0; 150 x 221: the SSIM H pass comes round again for 382 pixels
    assert 130 * 127 - eg == 126 and 150 * 221 - ss == 382 and 150 * 221 > 2 * eg


def test_the_entry_points_refuse_on_the_host_before_anything_is_launched():
    """-22 (SN_EINVAL) for a null pointer, a dtype outside 0 .. 2, an empty side, sums asked for without a place for them, and nothing asked for.  The
    pointers are host memory: a call that got as far as a launch would not return -22."""
    lib = L.load()
    arr = np.zeros(1 << 12, np.uint8)
    p = arr.ctypes.data
    a, b, c, d = p, p + 1024, p + 2048, p + 3072
    eg = [
        (None, 0, b, c, d, 1, 2, 2),                                                                              # null out
        (a, -1, b, c, d, 1, 2, 2), (a, 3, b, c, d, 1, 2, 2),                                                      # dtype
        (a, 0, b, c, d, 0, 2, 2), (a, 0, b, c, d, 1, 0, 2), (a, 0, b, c, d, 1, 2, 0), (a, 0, b, c, d, -1, 2, 2),  # T, H, W
        (a, 0, b, c, None, 1, 2, 2), (a, 0, b, None, None, 1, 2, 2),                                              # gt without sse
        (a, 0, None, None, d, 1, 2, 2), (a, 0, None, None, None, 1, 2, 2),                                        # neither img nor gt
    ]
    for args in eg:
        assert lib.sn_egress_u8(*args, None) == -22, args
    ss = [
        (None, 0, b, c, d, 1, 2, 2), (a, 0, None, c, d, 1, 2, 2),                                                 # null out, null gt
        (a, 0, b, None, d, 1, 2, 2), (a, 0, b, c, None, 1, 2, 2),                                                 # null scratch, null partial
        (a, -1, b, c, d, 1, 2, 2), (a, 3, b, c, d, 1, 2, 2),
        (a, 0, b, c, d, 0, 2, 2), (a, 0, b, c, d, 1, 0, 2), (a, 0, b, c, d, 1, 2, 0), (a, 0, b, c, d, 1, -3, 2),
    ]
    for args in ss:
        assert lib.sn_ssim_u8(*args, None) == -22, args
    ing = [
        (None, b, 0, 1, 2, 2), (a, None, 0, 1, 2, 2),                                                             # null src, null dst
        (a, b, -1, 1, 2, 2), (a, b, 3, 1, 2, 2),
        (a, b, 0, 0, 2, 2), (a, b, 0, 1, 0, 2), (a, b, 0, 1, 2, 0), (a, b, 0, 1, 2, -1),
    ]
    for args in ing:
        assert lib.sn_ingest_u8(*args, None) == -22, args
    assert not arr.any()
