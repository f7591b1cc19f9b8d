"""CPU tests of ``--despot``: the option's grammar and every refusal (shiftnet_amd/despot.py, the command line), the new symbol -- the header's
declaration, the ctypes signature, ABI 20, every SN_EINVAL of the entry point made with host pointers -- and, on the restatement
(tests/despot_ref.py), the exact properties the rule is chosen for.

The exact properties need no bound: on a static clip p == n == c off the dirt, so nothing is a seed and every byte leaves as it came, illegal codes
included; on a planted blotch of contrast above T every sample of it has a = b, |a| > T and |p - n| = 0, so it is a seed, an interior or edge sample
of a square of side >= 2 has at least three seeds around it (K <= 3), the grown mask adds only samples whose repair (p + n + 1) >> 1 = c is what
they held, and the clean clip comes back EXACTLY.  Shares measured on a pan and on noise are printed, never pinned."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import despot_ref as DR
import yuv_ref as R
from shiftnet_amd import despot as D
from shiftnet_amd import restore_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED)
F8_444 = R.Fmt(8, R.C444, R.BT709, R.FULL)
F10 = R.Fmt(10, R.C420_CENTER, R.BT709, R.LIMITED)
H, W = 48, 80


# ---- clips -------------------------------------------------------------------------------------------------------------------------------
def picture(fmt, seed, h=H, w=W, any_code=False):
    """One payload: a textured luma plane and smooth chroma; ``any_code``: every stored word, illegal codes included."""
    rng = np.random.default_rng(seed)
    top = (1 << fmt.bits) - 1
    s = 1 << (fmt.bits - 8)
    ch, cw = R.chroma_shape(fmt, h, w)
    if any_code:
        hi = 65535 if fmt.bits == 10 else 255
        return R.join_planes(rng.integers(0, hi + 1, (h, w)), rng.integers(0, hi + 1, (ch, cw)), rng.integers(0, hi + 1, (ch, cw)), fmt)
    y, x = np.mgrid[0:h, 0:w]
    Y = np.clip(np.floor((110 + 50 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0) + rng.normal(0, 4, (h, w))) * s), 16 * s, min(235 * s, top)).astype(np.int64)
    cy, cx = np.mgrid[0:ch, 0:cw]
    U = np.floor((128 + 30 * np.sin(cx / 9.0)) * s).astype(np.int64)
    V = np.floor((128 + 30 * np.cos(cy / 6.0)) * s).astype(np.int64)
    return R.join_planes(Y, U, V, fmt)


def plant(payload, fmt, squares, h=H, w=W):
    """The payload with square blotches (y, x, side, luma code in 8-bit codes), chroma pushed away too."""
    Y, U, V = (a.copy() for a in R.split_planes(payload, fmt, h, w))
    s = 1 << (fmt.bits - 8)
    sub = fmt.chroma != R.C444
    for y, x, side, code in squares:
        Y[y:y + side, x:x + side] = code * s
        ys, xs = (slice(y >> 1, (y + side + 1) >> 1), slice(x >> 1, (x + side + 1) >> 1)) if sub else (slice(y, y + side), slice(x, x + side))
        U[ys, xs] = 200 * s
        V[ys, xs] = 60 * s
    return R.join_planes(Y, U, V, fmt)


def squares_for(payload, fmt, seed, count=6, h=H, w=W, columns=None):
    """Up to ``count`` squares of side 2 .. 6 at code 20 or 235, whichever is further from what the picture holds there: contrast above 60.
    ``columns``: (first, past the last) column the squares lie in."""
    rng = np.random.default_rng(seed)
    Y = R.split_planes(payload, fmt, h, w)[0] >> (fmt.bits - 8)
    x_lo, x_hi = columns or (1, w - 1)
    out = []
    for _ in range(count):
        side = int(rng.integers(2, 7))
        y, x = int(rng.integers(1, h - side - 1)), int(rng.integers(x_lo, x_hi - side))
        out.append((y, x, side, 20 if Y[y:y + side, x:x + side].min() > 128 else 235))
    return [q for q in out if abs(int(Y[q[0]:q[0] + q[2], q[1]:q[1] + q[2]].max()) - q[3]) > 60 and abs(int(Y[q[0]:q[0] + q[2], q[1]:q[1] + q[2]].min()) - q[3]) > 60]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the rule's exact properties, on the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F8, F8_444, F10], ids=lambda f: "%d-%d-%d-%d" % f)
def test_a_static_clip_leaves_byte_for_byte_illegal_codes_included(fmt):
    for any_code in (False, True):
        clip = [picture(fmt, 3, any_code=any_code)] * 6
        for T, K, G in ((1, 0, 2), (24, 2, 1)):
            out, rec = DR.despot_stream_ref(clip, fmt, H, W, T=T, K=K, G=G)
            assert same(out, clip) and rec == [(0, 0, 0.0, False)] * 6


@pytest.mark.parametrize("fmt", [F8, F8_444, F10], ids=lambda f: "%d-%d-%d-%d" % f)
def test_planted_blotches_on_a_static_clip_come_back_as_the_clean_clip_exactly(fmt):
    clean = picture(fmt, 5)
    clip = [clean] * 7
    dirty = list(clip)
    planted = {}
    for f, columns in ((1, (1, 24)), (3, (28, 52)), (5, (56, 79))):    # interior frames between clean ones, their squares in columns of their own: p == n
        sq = squares_for(clean, fmt, seed=f, columns=columns)
        assert sq
        planted[f] = sq
        dirty[f] = plant(clean, fmt, sq)
    assert not same(dirty, clip)
    for K in (0, 2, 3):
        for G in (0, 1, 2):
            for chroma in ("follow", "off"):
                out, rec = DR.despot_stream_ref(dirty, fmt, H, W, T=24, K=K, G=G, chroma=chroma, max_share=0.5)
                for f in range(7):
                    Y, U, V = R.split_planes(out[f], fmt, H, W)
                    Yc, Uc, Vc = R.split_planes(clean, fmt, H, W)
                    assert np.array_equal(Y, Yc), (K, G, chroma, f)
                    if chroma == "follow":
                        assert np.array_equal(U, Uc) and np.array_equal(V, Vc), (K, G, f)
                    else:                                           # chroma left alone: the dirt's chroma stays
                        lb = H * W * (1 if fmt.bits == 8 else 2)
                        assert np.array_equal(out[f][lb:], dirty[f][lb:])
                for f, sq in planted.items():
                    area = sum(side * side for _, _, side, _ in sq)     # squares may overlap: at most their samples, at least one square's
                    assert 4 <= rec[f][0] <= area and rec[f][1] >= rec[f][0] and not rec[f][3]
                assert rec[0] == rec[2] == rec[4] == rec[6] == (0, 0, 0.0, False)


def test_an_unlisted_hard_cut_between_static_scenes_leaves_byte_for_byte():
    a, b = picture(F8, 1), picture(F8, 2, any_code=True)
    clip = [a] * 4 + [b] * 4
    out, rec = DR.despot_stream_ref(clip, F8, H, W, T=1, K=0, G=2)         # at either side of the cut one of a, b is 0
    assert same(out, clip) and all(r == (0, 0, 0.0, False) for r in rec)


def test_a_flash_frame_is_kept_and_the_ends_of_clips_and_listed_scenes_are_the_sources():
    base = picture(F8, 4)
    Y, U, V = R.split_planes(base, F8, H, W)
    flash = R.join_planes(np.minimum(Y + 90, 255), U, V, F8)
    clip = [base] * 3 + [flash] + [base] * 3
    out, rec = DR.despot_stream_ref(clip, F8, H, W, T=24, K=2, G=1, max_share=0.05)
    assert same(out, clip) and rec[3][3] and rec[3][2] > 0.05 and rec[3][1] == round(rec[3][2] * H * W)
    assert [r[3] for r in rec] == [False] * 3 + [True] + [False] * 3
    out, rec = DR.despot_stream_ref(clip, F8, H, W, T=24, K=2, G=1, max_share=1.0)      # without the guard the flash is repaired away
    assert not rec[3][3] and rec[3][2] > 0.05 and not np.array_equal(out[3], clip[3])
    # dirt in the first and last frame of the stream, and on either side of a listed cut, stays: those frames have one neighbour
    sq = squares_for(base, F8, seed=9)
    d = plant(base, F8, sq)
    clip = [d, base, d, d, base, d, base, d]
    out, rec = DR.despot_stream_ref(clip, F8, H, W, cuts=[3], T=24, K=2, G=1, max_share=0.5)
    for f in (0, 2, 3, 7):
        assert np.array_equal(out[f], clip[f]) and rec[f] == (0, 0, 0.0, False)
    assert np.array_equal(out[5], base) and rec[5][0] > 0                 # ... and inside the scene it goes
    whole, _ = DR.despot_stream_ref(clip, F8, H, W, cuts=(), T=24, K=2, G=1, max_share=0.5)
    assert np.array_equal(whole[7], clip[7]) and np.array_equal(whole[0], clip[0])


def moving(fmt, frames, vy, vx, seed=7, h=H, w=W):
    """A pan by (vy, vx) samples per frame over a larger texture (luma and, at 4:4:4, chroma alike)."""
    rng = np.random.default_rng(seed)
    big = np.clip(120 + 45 * np.sin(np.arange(w + 64)[None, :] / 6.0) * np.cos(np.arange(h + 64)[:, None] / 4.0) + rng.normal(0, 6, (h + 64, w + 64)), 16, 235)
    big = np.floor(big).astype(np.int64)
    ch, cw = R.chroma_shape(fmt, h, w)
    out = []
    for t in range(frames):
        y0, x0 = 32 + vy * t, 32 + vx * t                            # |v| t <= 32: inside the texture
        out.append(R.join_planes(big[y0:y0 + h, x0:x0 + w], np.full((ch, cw), 128), np.full((ch, cw), 128), fmt))
    return out


def test_the_result_does_not_depend_on_the_chunk_length():
    clip = moving(F8, 9, 1, 2)
    for f in (2, 5, 6):
        clip[f] = plant(clip[f], F8, squares_for(clip[f], F8, seed=f))
    ref, rrec = DR.despot_stream_ref(clip, F8, H, W, cuts=[4], T=24, K=2, G=1)
    for chunk in (1, 2, 3, 16):
        out, rec = DR.despot_stream_ref(clip, F8, H, W, cuts=[4], T=24, K=2, G=1, chunk=chunk)
        assert same(out, ref) and rec == rrec


def test_on_a_pan_with_planted_blotches_the_hit_and_false_shares_are_printed():
    h, w = 96, 160
    clean = moving(F8, 7, 2, -3, h=h, w=w)
    dirty = list(clean)
    mask = {}
    for f in range(1, 6):
        sq = squares_for(clean[f], F8, seed=20 + f, count=8, h=h, w=w)
        dirty[f] = plant(clean[f], F8, sq, h=h, w=w)
        m = np.zeros((h, w), bool)
        for y, x, side, _ in sq:
            m[y:y + side, x:x + side] = True
        mask[f] = m
    out, rec = DR.despot_stream_ref(dirty, F8, h, w, T=24, K=2, G=1, max_share=0.5)
    hit = planted = false = clean_samples = 0
    for f, m in mask.items():
        changed = out[f][:h * w].reshape(h, w) != dirty[f][:h * w].reshape(h, w)
        hit, planted = hit + int((changed & m).sum()), planted + int(m.sum())
        false, clean_samples = false + int((changed & ~m).sum()), clean_samples + int((~m).sum())
    print(f"pan by (2, -3) per frame, 96 x 160, T 24, K 2, G 1: {hit} of {planted} planted samples changed (hit share {hit / planted:.4f}), "
          f"{false} of {clean_samples} other samples changed (false share {false / clean_samples:.6f}); records {rec}")
    assert planted > 0                                              # measured and printed, not pinned


def test_the_defaults_on_noise_and_on_planted_squares_are_printed():
    """What T = 24, K = 2, G = 1 gives on a noise-only static clip (180 x 320, zero motion, i.i.d. luma noise) and on 20 planted squares of side
    2 .. 6 at codes 20 / 235: re-measured here on the restatement and printed, not asserted."""
    h, w = 180, 320
    rng = np.random.default_rng(0)
    base = picture(F8, 6, h=h, w=w)
    Y, U, V = R.split_planes(base, F8, h, w)
    for sigma in (5, 10, 20):
        clip = [R.join_planes(np.clip(np.rint(Y + rng.normal(0, sigma, (h, w))), 0, 255).astype(np.int64), U, V, F8) for _ in range(3)]
        _, rec = DR.despot_stream_ref(clip, F8, h, w, T=24, K=2, G=1, max_share=1.0)
        print(f"noise only, sigma {sigma}: share replaced {rec[1][2]:.6f} ({rec[1][0]} core seeds)")
    sq = squares_for(base, F8, seed=3, count=20, h=h, w=w)
    clip = [base, plant(base, F8, sq, h=h, w=w), base]
    out, rec = DR.despot_stream_ref(clip, F8, h, w, T=24, K=2, G=1, max_share=1.0)
    left = int((out[1][:h * w] != base[:h * w]).sum())
    print(f"{len(sq)} planted squares on a static clip: {left} luma samples differ from the clean frame afterwards; record {rec[1]}")


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_the_grammar_and_the_refusals():
    assert D.parse_despot("24") == 24 and D.parse_despot(" 255 ") == 255 and D.parse_despot("1") == 1
    for bad in ("0", "256", "-1", "2.5", "", "auto"):
        with pytest.raises(ValueError):
            D.parse_despot(bad)
    assert D.despot_form(None) == (None, 2, 1, "follow", 0.05) and D.despot_form(24) == (24, 2, 1, "follow", 0.05)
    assert D.despot_form(255, 0, 2, "off", 1) == (255, 0, 2, "off", 1.0) and D.despot_form(1, 8, 0, "follow", 0.5) == (1, 8, 0, "follow", 0.5)
    for bad in (0, 256, -1, 2.5, "24", True):
        with pytest.raises(ValueError, match="despot must be"):
            D.despot_form(bad)
    for bad in (-1, 9, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="despot_support"):
            D.despot_form(24, bad)
    for bad in (-1, 3, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="despot_grow"):
            D.despot_form(24, 2, bad)
    for bad in ("mean", "gain", None, 1):
        with pytest.raises(ValueError, match="despot_chroma"):
            D.despot_form(24, 2, 1, bad)
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), "0.05", True, None):
        with pytest.raises(ValueError, match="despot_max_share"):
            D.despot_form(24, 2, 1, "follow", bad)
    for kw, word in ((dict(support=3), "despot_support"), (dict(grow=2), "despot_grow"), (dict(chroma="off"), "despot_chroma"),
                     (dict(max_share=0.1), "despot_max_share")):
        with pytest.raises(ValueError, match=word + ".*needs despot"):
            D.despot_form(None, **kw)
    with pytest.raises(ValueError, match="despot together with add_noise"):
        D.despot_form(24, add_noise=[5.0] * 16)
    with pytest.raises(ValueError, match="despot together with add_blur"):
        D.despot_form(24, add_blur=7)
    assert D.despot_form(None, add_noise=[5.0] * 16, add_blur=7) == (None, 2, 1, "follow", 0.05)      # without the option nothing of it is judged
    assert D.frame_record(3, 10, 200, 0.05) == (3, 10, 0.05, False) and D.frame_record(3, 11, 200, 0.05) == (3, 11, 0.055, True)
    frames = [(0, 0, 0.0, False), (20, 42, 0.013676, False), (900, 3000, 0.78125, True), (0, 0, 0.0, False)]
    assert D.median_share(frames) == 0.006838 and D.frames_kept(frames) == 1 and D.median_share([]) == 0.0
    text = D.format_despot(frames)
    assert text.splitlines()[:3] == ["0 0 0.000000 0", "20 42 0.013676 0", "900 3000 0.781250 1"] and len(text.splitlines()) == 5
    assert text.splitlines()[-1] == "# median share replaced: 0.006838; frames kept as they came (the guard): 1"


def test_the_command_line_takes_the_options_and_refuses_what_does_not_go_together(capsys):
    ap = restore_cli.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["in.y4m", "out.y4m"])
    assert (a.despot, a.despot_support, a.despot_grow, a.despot_chroma, a.despot_max_share, a.despot_out) == (None, 2, 1, "follow", 0.05, None)
    a = ap.parse_args(base + ["--despot", "24", "--despot_support", "3", "--despot_grow", "2", "--despot_chroma", "off", "--despot_max_share", "0.1",
                              "--despot_out", "d.txt", "in.y4m", "out.y4m"])
    assert (a.despot, a.despot_support, a.despot_grow, a.despot_chroma, a.despot_max_share, a.despot_out) == (24, 3, 2, "off", 0.1, "d.txt")
    for more, word in ((["--despot", "0"], "--despot"), (["--despot", "256"], "--despot"), (["--despot", "24", "--despot_chroma", "gain"], "--despot_chroma")):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(base + more + ["in.y4m", "out.y4m"])
        assert e.value.code == 2 and word in capsys.readouterr().err
    gone = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]          # judged before any file is opened
    for more, words in ((["--despot", "24", "--add_noise", "5"], ["--despot", "--add_noise"]),
                        (["--despot", "24", "--add_blur", "7"], ["--despot", "--add_blur"]),
                        (["--despot_out", "/nonexistent/d.txt"], ["--despot_out needs --despot"]),
                        (["--despot_chroma", "off"], ["needs despot"]), (["--despot_grow", "2"], ["needs despot"]),
                        (["--despot", "24", "--despot_support", "9"], ["despot_support"]), (["--despot", "24", "--despot_grow", "3"], ["despot_grow"]),
                        (["--despot", "24", "--despot_max_share", "0"], ["despot_max_share"])):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + more + gone)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (more, err)


def test_header_build_list_and_library_have_the_new_symbol_and_the_entry_point_refuses_on_the_host():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_despot.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_despot.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    from shiftnet_amd.io_edges import yuv_fmt
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^int sn_yuv_despot\(const uint8_t\* src, const sn_yuv_fmt\* fmt, const int8_t\* mv_prev, const int8_t\* mv_next, uint8_t\* dst, "
                     r"uint32_t\* counts /\* \[n\]\[2\] \*/,\s+int S, int f0, int n, int threshold /\* in the format's codes \*/, int support, int grow, "
                     r"int chroma /\* 0 off, 1 follow \*/,\s+int H, int W, void\* stream\);", header, flags=re.M)
    assert "tests/despot_ref.py" in header
    vp, ci = C.c_void_p, C.c_int
    assert hasattr(lib, "sn_yuv_despot") and "sn_yuv_despot" in L.SYMBOLS
    assert lib.sn_yuv_despot.argtypes == [vp, C.POINTER(L.YuvFmt), vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp] and lib.sn_yuv_despot.restype is ci
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    # the argument checks are host side and need no GPU: host memory is refused before anything would read it
    arr = np.zeros(1 << 21, np.uint8)
    buf = arr.ctypes.data + (-arr.ctypes.data) % 16
    src, dst, mvp, mvn, cnt = buf, buf + (1 << 20), buf + (3 << 19), buf + (3 << 19) + 4096, buf + (3 << 19) + 8192
    f8, f10 = yuv_fmt(8, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED), yuv_fmt(10, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    fb8 = f8.frame_bytes(40, 72)                                     # 5 payloads of 40 x 72 at 4:4:4 are 43200 bytes: far below 2^20
    good = dict(src=src, fmt=f8, mv_prev=mvp, mv_next=mvn, dst=dst, counts=cnt, S=5, f0=1, n=3, threshold=24, support=2, grow=1, chroma=1, H=40, W=72)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.sn_yuv_despot(a["src"], a["fmt"], a["mv_prev"], a["mv_next"], a["dst"], a["counts"], a["S"], a["f0"], a["n"], a["threshold"],
                                 a["support"], a["grow"], a["chroma"], a["H"], a["W"], None)

    bad = [dict(src=None), dict(fmt=None), dict(mv_prev=None), dict(mv_next=None), dict(dst=None), dict(counts=None)]      # null pointers
    bad += [dict(fmt=f) for f in (yuv_fmt(12, 0, 0, 0), yuv_fmt(8, 3, 0, 0), yuv_fmt(8, 0, 2, 0), yuv_fmt(8, 0, 0, 2))]      # bits, chroma code, matrix, range
    bad += [dict(fmt=f10, src=src + 1), dict(fmt=f10, dst=dst + 1)]                                     # 10 bit: a payload at an odd address
    bad += [dict(counts=cnt + 1), dict(counts=cnt + 2)]                                                 # counts is uint32
    bad += [dict(S=0), dict(S=65536), dict(H=0), dict(W=0)]
    bad += [dict(f0=0), dict(f0=-1), dict(n=0), dict(n=-1), dict(f0=1, n=4), dict(f0=2, n=3), dict(f0=4, n=1), dict(S=2, f0=1, n=1)]      # f0 + n > S - 1
    bad += [dict(threshold=-1), dict(support=-1), dict(support=9), dict(grow=-1), dict(grow=3), dict(chroma=-1), dict(chroma=2)]
    bad += [dict(dst=src), dict(dst=src + fb8), dict(dst=src + 5 * fb8 - 1), dict(dst=src - 3 * fb8 + 1), dict(dst=src + 2 * fb8 + 1)]      # dst overlaps src
    bad += [dict(H=32 * 65535 + 1, W=8, dst=src + (1 << 40))]                                           # more rows of workgroups than a grid has
    for kw in bad:
        assert call(**kw) == -22, kw
