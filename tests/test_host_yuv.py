"""CPU: the Y4M container, the window planner of the video restorer, and the float32 restatement of the Y'CbCr kernels
(tests/yuv_ref.py ``*_emu``, which the GPU tests require the kernels to equal bit for bit) against the BT.601 / BT.709 definition in
float64 (``*_f64``)."""
import ctypes
import io
import itertools
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import yuv_ref as R
from shiftnet_amd import restore, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [R.Fmt(bits, R.C444, m, r) for bits in (8, 10) for m in (R.BT601, R.BT709) for r in (R.LIMITED, R.FULL)]
CASE_IDS = [f"{f.bits}bit-{'709' if f.matrix else '601'}-{'full' if f.range else 'limited'}" for f in CASES]
N10 = 20_000_000


def triples(bits):
    """All 2^24 8-bit triples, or 2e7 random 10-bit triples, in chunks."""
    if bits == 8:
        a = np.arange(256, dtype=np.int64)
        for y0 in range(0, 256, 64):
            Y, U, V = np.meshgrid(a[y0:y0 + 64], a, a, indexing="ij")
            yield Y.ravel(), U.ravel(), V.ravel()
    else:
        rng = np.random.default_rng(10)
        for _ in range(5):
            yield tuple(rng.integers(0, 1024, (3, N10 // 5)))


# ---- Y4M ----------------------------------------------------------------------------------------------------------------------------
def _payloads(hd, n, seed=0):
    rng = np.random.default_rng(seed)
    if hd.bits == 8:
        return [rng.integers(0, 256, hd.frame_bytes, dtype=np.uint8) for _ in range(n)]
    return [rng.integers(0, 1024, hd.frame_bytes // 2).astype("<u2").view(np.uint8) for _ in range(n)]


@pytest.mark.parametrize("mode", sorted(y4m.MODES))
@pytest.mark.parametrize("hw", [(36, 52), (7, 13), (1, 1)])
def test_y4m_write_then_read_gives_the_same_header_and_bytes(mode, hw):
    hd = y4m.Y4MHeader(width=hw[1], height=hw[0], fps="30000:1001", aspect="1:1", chroma=mode, extensions=["COLORRANGE=FULL"])
    c = (hw[0] * hw[1]) if y4m.MODES[mode][1] == 0 else ((hw[0] + 1) // 2) * ((hw[1] + 1) // 2)
    assert hd.frame_bytes == (hw[0] * hw[1] + 2 * c) * (1 if y4m.MODES[mode][0] == 8 else 2)
    frames = _payloads(hd, 3)
    f = io.BytesIO()
    w = y4m.Y4MWriter(f, hd)
    for p in frames:
        w.write(p)
    rd = y4m.Y4MReader(io.BytesIO(f.getvalue()))
    g = rd.header
    assert (g.width, g.height, g.fps, g.interlace, g.aspect, g.chroma, g.extensions) == (hw[1], hw[0], "30000:1001", "p", "1:1", mode, ["COLORRANGE=FULL"])
    assert g.color_range == "full" and g.bits == y4m.MODES[mode][0]
    got = list(rd)
    assert len(got) == 3 and all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(got, frames))


def test_y4m_reads_from_a_pipe_that_cannot_seek():
    hd = y4m.Y4MHeader(width=101, height=67, chroma="420mpeg2")
    frames = _payloads(hd, 4, seed=1)
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, "wb", buffering=0) as fw:       # unbuffered and in small pieces: the reader sees short reads
            buf = io.BytesIO()
            wr = y4m.Y4MWriter(buf, hd)
            for p in frames:
                wr.write(p)
            data = buf.getvalue()
            for o in range(0, len(data), 1000):
                fw.write(data[o:o + 1000])
    th = threading.Thread(target=feed)
    th.start()
    with os.fdopen(r, "rb", buffering=0) as fr:
        assert not fr.seekable()
        rd = y4m.Y4MReader(fr)
        got = list(rd)
    th.join()
    assert rd.header.color_range is None
    assert len(got) == 4 and all(np.array_equal(a, b) for a, b in zip(got, frames))


@pytest.mark.parametrize("line,word", [(b"YUV4MPEG2 W4 H4 F25:1 It A1:1 C420jpeg\n", "It"), (b"YUV4MPEG2 W4 H4 F25:1 Ip C422\n", "C422"),
                                       (b"YUV4MPEG2 W4 H4 F25:1 Ip C420p12\n", "C420p12"), (b"YUV4MPEG2 W4 H4 Ib Cmono\n", "Ib")])
def test_y4m_refuses_interlaced_and_unknown_chroma_and_names_the_tag(line, word):
    with pytest.raises(y4m.Y4MError) as e:
        y4m.Y4MReader(io.BytesIO(line))
    assert word in str(e.value)


def test_y4m_truncated_frame_raises():
    hd = y4m.Y4MHeader(width=8, height=8)
    f = io.BytesIO()
    y4m.Y4MWriter(f, hd).write(_payloads(hd, 1)[0])
    with pytest.raises(y4m.Y4MError):
        list(y4m.Y4MReader(io.BytesIO(f.getvalue()[:-5])))


# ---- planner --------------------------------------------------------------------------------------------------------------------------
def test_planner_restores_every_frame_once_in_order_with_indices_inside_the_clip():
    for n, L in itertools.product(range(1, 41), range(1, 18)):
        plan = restore.plan_windows(n, L)
        done = []
        for k, (lo, cnt, idx) in enumerate(plan):
            assert lo == k * L and 1 <= cnt <= L and len(idx) == 2 + cnt + 2
            assert all(0 <= i < n for i in idx)
            assert idx[2:2 + cnt] == list(range(lo, lo + cnt))
            for j, i in enumerate(idx):                                     # inside the clip an input index is the frame itself
                want = lo - 2 + j
                if 0 <= want < n:
                    assert i == want
            done += idx[2:2 + cnt]
        assert done == list(range(n)), (n, L)
        assert all(cnt == L for _, cnt, _ in plan[:-1])


def test_planner_reflects_without_repeating_the_edge_and_clamps_short_clips():
    assert restore.plan_windows(11, 4)[0][2] == [2, 1, 0, 1, 2, 3, 4, 5]
    assert restore.plan_windows(11, 4)[2][2] == [6, 7, 8, 9, 10, 9, 8]       # N -> N - 2, N + 1 -> N - 3
    assert restore.plan_windows(10, 5)[1][2] == [3, 4, 5, 6, 7, 8, 9, 8, 7]
    assert [restore.reflect_index(i, 7) for i in (-2, -1, 0, 6, 7, 8)] == [2, 1, 0, 6, 5, 4]
    assert restore.plan_windows(1, 4) == [(0, 1, [0, 0, 0, 0, 0])]
    assert restore.plan_windows(2, 4) == [(0, 2, [0, 0, 0, 1, 1, 1])]
    assert restore.plan_windows(3, 1)[0][2] == [2, 1, 0, 1, 2] and restore.plan_windows(3, 1)[2][2] == [0, 1, 2, 1, 0]


def test_frame_source_with_unknown_length_gives_the_planned_windows():
    """The restorer reads ahead on an iterator (a pipe: N unknown until it ends); its windows are the planner's."""
    for n, L in itertools.product((1, 2, 3, 5, 11, 16, 17, 33), (1, 4, 16)):
        src = restore._Frames(iter([np.array([i]) for i in range(n)]))
        got, k = [], 0
        while True:
            w = src.window(k, L)
            if w is None:
                break
            got.append((w[0], w[1], [int(f[0]) for f in w[2]]))
            assert len(src.buf) <= L + 2 * (restore.PAST + restore.FUTURE)            # the look-ahead stays bounded
            k += 1
        assert got == restore.plan_windows(n, L), (n, L)


def test_padded_sizes_follow_the_variant():
    assert restore.padded_size(100, 108, "plus") == (104, 112) and restore.padded_size(100, 108, "small") == (100, 108)
    assert restore.padded_size(67, 101, "small") == (68, 104) and restore.padded_size(720, 1280, "plus") == (720, 1280)


# ---- arithmetic: emu (float32, the kernel's order) against the definition in float64 ---------------------------------------------------
@pytest.mark.parametrize("fmt", CASES, ids=CASE_IDS)
def test_ingest_emu_is_within_1e_6_of_the_float64_definition(fmt):
    """Measured (unclamped RGB, all 2^24 8-bit / 2e7 random 10-bit triples): see DESIGN.md 3.11.  The bound is 1/1000 of a 10-bit code."""
    worst = 0.0
    for Y, U, V in triples(fmt.bits):
        d = np.abs(R.yuv_to_rgb_emu(Y, U, V, 1, fmt, clamp=False).astype(np.float64) - R.yuv_to_rgb_f64(Y, U, V, fmt))
        worst = max(worst, float(d.max()))
    print(f"ingest emu vs f64 {fmt}: max |RGB32 - RGB64| = {worst:.3e}")
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("chroma", [R.C420_CENTER, R.C420_LEFT])
def test_upsampled_ingest_emu_is_within_1e_6_of_float64_bilinear(chroma):
    """Whole frames with odd sizes and padding: the integer 9/3/3/1 (3/1 x 1|1,1) numerators against float64 bilinear weights."""
    rng = np.random.default_rng(3)
    for bits, H, W in ((8, 67, 101), (10, 36, 52), (8, 1, 1), (8, 2, 3)):
        fmt = R.Fmt(bits, chroma, R.BT709, R.LIMITED)
        p = rng.integers(0, 1 << bits, (2, R.frame_bytes(fmt, H, W) // (bits // 8 if bits == 8 else 2)))
        p = p.astype(np.uint8) if bits == 8 else p.astype("<u2").view(np.uint8).reshape(2, -1)
        a = R.ingest_emu(p, fmt, H, W, H + 5, W + 3).astype(np.float64)
        b = R.ingest_f64(p, fmt, H, W, H + 5, W + 3)
        assert np.abs(a - b).max() <= 1e-6
        assert np.array_equal(a[:, :, H:, :], np.broadcast_to(a[:, :, H - 1:H, :], a[:, :, H:, :].shape))      # padding = the edge pixel
        assert np.array_equal(a[:, :, :, W:], np.broadcast_to(a[:, :, :, W - 1:W], a[:, :, :, W:].shape))
    # siting, on a horizontal ramp: centre-sited chroma i sits at luma 2i + 0.5, left-sited at 2i
    fmt = R.Fmt(8, chroma, R.BT601, R.FULL)
    U = np.tile(np.arange(8) * 16, (4, 1))
    num, den = R.upsample_num(U, chroma, np.arange(8), np.arange(16))
    x = np.arange(16)
    want = np.clip((x - 0.5) / 2, 0, 7) * 16 if chroma == R.C420_CENTER else np.clip(x / 2, 0, 7) * 16
    assert np.array_equal(num[3] / den, want)


@pytest.mark.parametrize("fmt", CASES, ids=CASE_IDS)
def test_egress_emu_codes_differ_from_float64_by_at_most_one_and_only_next_to_a_tie(fmt):
    rng = np.random.default_rng(20 + fmt.bits + fmt.matrix * 2 + fmt.range)
    for _ in range(4):
        rgb = (rng.random((3, 5_000_000), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
        _, q32 = R.rgb_to_yuv444_emu(rgb, fmt)
        raw64, q64 = R.rgb_to_yuv444_f64(rgb, fmt)
        diff = q32 != q64
        assert np.abs(q32 - q64).max() <= 1
        frac = np.abs(raw64 - np.floor(raw64) - 0.5)              # distance of the float64 value from the tie between two codes
        assert diff.sum() == 0 or float(frac[diff].max()) <= 1e-3, float(frac[diff].max())


@pytest.mark.parametrize("chroma", [R.C420_CENTER, R.C420_LEFT])
def test_subsampled_egress_emu_matches_float64(chroma):
    rng = np.random.default_rng(4)
    for bits, H, W in ((8, 67, 101), (10, 36, 52), (8, 1, 1)):
        fmt = R.Fmt(bits, chroma, R.BT601, R.LIMITED)
        x = (rng.random((2, 3, H + 1, W + 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
        a, b = R.egress_emu(x, fmt, H, W), R.egress_f64(x, fmt, H, W)
        assert a.shape == (2, R.frame_bytes(fmt, H, W)) and a.dtype == np.uint8
        va, vb = (a.view("<u2"), b.view("<u2")) if bits == 10 else (a, b)
        assert np.abs(va.astype(np.int64) - vb.astype(np.int64)).max() <= 1


@pytest.mark.parametrize("fmt", CASES, ids=CASE_IDS)
def test_round_trip_returns_every_in_gamut_triple_exactly(fmt):
    total = ingamut = 0
    worst = 0.0
    for Y, U, V in triples(fmt.bits):
        rgb64 = R.yuv_to_rgb_f64(Y, U, V, fmt)
        ok = (rgb64.min(0) >= 0.0) & (rgb64.max(0) <= 1.0)
        Y, U, V = Y[ok], U[ok], V[ok]
        raw, q = R.rgb_to_yuv444_emu(R.yuv_to_rgb_emu(Y, U, V, 1, fmt), fmt)
        assert np.array_equal(q[0], Y) and np.array_equal(q[1], U) and np.array_equal(q[2], V)
        worst = max(worst, float(np.abs(raw - np.rint(raw)).max()))
        total += ok.size
        ingamut += int(ok.sum())
    share = ingamut / total
    print(f"round trip {fmt}: in-gamut share {share:.4f}, max distance from an integer before rounding {worst:.2e}")
    assert 0.15 <= share <= 0.25, share          # the set is large: 15.5 % .. 24.2 % of all triples
    assert worst <= 1e-3                         # a few float32 roundings at magnitude <= 1023 (ulp 6.1e-5): far from any tie


def test_dtype_rounding_helpers_agree_with_torch():
    import torch
    x = np.random.default_rng(5).random(100000, dtype=np.float32)
    assert np.array_equal(R.to_dtype_bits(x, "bf16"), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.to_dtype_bits(x, "fp16"), torch.from_numpy(x).to(torch.float16).numpy())


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_yuv_entry_points_and_keeps_the_abi_version():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_yuv.hip" in mod.SOURCES
    csrc = os.path.join(ROOT, "shift-net_amd", "csrc")           # a unit left out of the build would only show as a missing symbol on the GPU
    assert len(mod.SOURCES) == len(set(mod.SOURCES)) and set(mod.SOURCES) == {f for f in os.listdir(csrc) if f.endswith(".hip")}
    mod.build()                                              # hipcc cross-compiles gfx950 without a GPU
    from shiftnet_amd import lib as L
    lib = L.load()
    assert hasattr(lib, "sn_ingest_yuv") and hasattr(lib, "sn_egress_yuv")
    assert "sn_ingest_yuv" in L.SYMBOLS and "sn_egress_yuv" in L.SYMBOLS
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        open(src, "w").write('#include <stdio.h>\n#include "shiftnet_hip.h"\nint main(void){printf("%zu\\n", sizeof(sn_yuv_fmt));return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        assert int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout) == ctypes.sizeof(L.YuvFmt)
    for f in CASES:
        assert L.YuvFmt(*f).frame_bytes(67, 101) == R.frame_bytes(f, 67, 101)
    assert L.YuvFmt(8, L.SN_YUV_420_CENTER, 0, 0).frame_bytes(67, 101) == 67 * 101 + 2 * 34 * 51
    assert (L.SN_YUV_444, L.SN_YUV_420_CENTER, L.SN_YUV_420_LEFT, L.SN_YUV_BT601, L.SN_YUV_BT709, L.SN_YUV_LIMITED, L.SN_YUV_FULL) == \
           (R.C444, R.C420_CENTER, R.C420_LEFT, R.BT601, R.BT709, R.LIMITED, R.FULL)


def test_restore_cli_parser_and_sigma_rule():
    ap = restore.make_parser()
    a = ap.parse_args(["--variant", "deblur_small", "--checkpoint", "synthetic", "-", "-"])
    assert (a.dtype, a.one_len, a.matrix, a.range, a.no_pipeline, a.input, a.output) == ("bf16", 16, None, None, False, "-", "-")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "denoise_small", "--checkpoint", "synthetic",
                        "-", "-"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--sigma" in r.stderr
