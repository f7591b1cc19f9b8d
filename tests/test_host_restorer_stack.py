"""No device: what tests/test_gpu_restorer_stack.py stands on.  The three option stacks of tests/stack_cases.py pass the constructor's argument checks
and every refusal between their options is a ValueError; the restatement's plan (tests/time_ref.py), from which the GPU file takes a frame's window and
its number in its scene, is the product's plan; and the two references that the picture identity compares on the full frame and on the cropped
stream -- the grain's and the difference sums' -- agree with each other there."""
import types

import numpy as np
import pytest

import diff_stats_ref as D
import grain_ref as GR
import picture_ref as P
import stack_cases as S
import time_ref as TR
import yuv_ref as R
from shiftnet_amd import grain, restore, windows


class _Net:
    """As much of a GShiftNet as VideoRestorer looks at.  ``cuda``: the parameter claims a HIP device, so that the checks behind the device check are
    reached as well; nothing is allocated as long as ``window_overlap`` stays off (its weights are the one thing the constructor puts on the device)."""

    def __init__(self, denoise, cuda=False):
        self.V = types.SimpleNamespace(denoise=denoise, topo="small")
        self.cuda = cuda

    def parameters(self):
        import torch
        if self.cuda:
            return iter([types.SimpleNamespace(device=types.SimpleNamespace(type="cuda"), dtype=torch.bfloat16)])
        return iter([torch.zeros(1)])


@pytest.fixture(scope="module", params=list(S.STACKS))
def st(request):
    return S.STACKS[request.param]()


def build(st, cuda=False, **more):
    kw = dict(st.kw, **more)
    if cuda:
        kw.pop("window_overlap")
    return restore.VideoRestorer(_Net(st.variant.startswith("denoise"), cuda), S.ONE_LEN, **kw)


def test_the_stacks_pass_every_argument_check(st):
    with pytest.raises(ValueError, match="HIP device"):           # the last thing the constructor asks before it builds its parts
        build(st)
    vr = build(st, cuda=True)                                      # ... and the checks behind it pass too
    assert (vr.add_noise is not None) + (vr.add_blur is not None) + (vr.deflicker is not None) == 1
    assert len(st.pay) == 11 and all(p.size == R.frame_bytes(st.fmt, st.h, st.w) for p in st.pay)
    assert st.gt is None or all(p.size == R.frame_bytes(st.ofmt, st.h, st.w) for p in st.gt)


def test_the_three_stacks_cover_every_chroma_layout_and_both_bit_depths():
    fmts = [S.STACKS[n]().fmt for n in S.STACKS]
    assert {f.chroma for f in fmts} == {R.C444, R.C420_CENTER, R.C420_LEFT} and {f.bits for f in fmts} == {8, 10}


REFUSALS = [("D", dict(ensemble=2), r"ensemble.*tile"), ("D", dict(add_noise=5.0), r"deflicker together with add_noise"),
            ("D", dict(add_blur=3), r"deflicker together with add_blur"), ("D", dict(view="removed"), r"view"),
            ("E", dict(tile=(16, 16), tile_overlap=4), r"ensemble.*tile"), ("E", dict(add_blur=3), r"add_blur together with add_noise"),
            ("E", dict(deflicker=2), r"deflicker together with add_noise"), ("E", dict(view="removed"), r"view"),
            ("B", dict(tile=(16, 16), tile_overlap=4), r"ensemble.*tile"), ("B", dict(add_noise=5.0), r"add_blur together with add_noise"),
            ("B", dict(deflicker=2), r"deflicker together with add_blur"), ("B", dict(grain=4.0), r"grain.*view"), ("B", dict(report=True), r"report.*view"),
            ("B", dict(amount=0.5), r"view"), ("B", dict(sigma="auto"), r"denoise variants"), ("B", dict(noise_model="level"), r"denoise variants"),
            ("B", dict(view=None, grain="auto"), r"grain='auto'.*deblur")]


@pytest.mark.parametrize("name,more,match", REFUSALS, ids=[f"{n}+{'+'.join(m)}" for n, m, _ in REFUSALS])
def test_every_refusal_between_the_stacks_options_is_a_value_error(name, more, match):
    with pytest.raises(ValueError, match=match):
        build(S.STACKS[name](), cuda=True, **more)


def test_the_restatements_plan_is_the_products_for_every_stack(st):
    n = len(st.pay)
    for cuts in (st.cuts, []):
        assert TR.scene_plan(n, S.ONE_LEN, cuts, st.V) == windows.plan_scene_overlap_windows(n, S.ONE_LEN, cuts, st.V)
    for a, b in zip([0] + st.cuts, st.cuts + [n]):               # ... and a scene's slice has the plan of a stream of its own
        assert TR.scene_plan(b - a, S.ONE_LEN, [], st.V) == windows.plan_overlap_windows(b - a, S.ONE_LEN, st.V)


def test_the_frame_maps_agree_with_the_plan(st):
    n = len(st.pay)
    frames, wins = S.frame_maps(n, st.cuts, st.V)
    plan = windows.plan_scene_overlap_windows(n, S.ONE_LEN, st.cuts, st.V)
    assert len(wins) == len(plan) and [w[1] for w in wins] == [p[4] for p in plan] and sum(w[1] for w in wins) == n
    for f, (k, number) in enumerate(frames):
        lo, cnt, idx, head, written = plan[k]
        scene = max([0] + [c for c in st.cuts if c <= f])
        assert lo <= f < lo + written and number == f - scene and wins[k] == (lo, written, scene)
        assert idx[windows.PAST + f - lo] == f                     # the window's own frame f is that input frame
    assert [k for k, _ in frames] == sorted(k for k, _ in frames) and {k for k, _ in frames} == set(range(len(plan)))
    assert any(number != f for f, (_, number) in enumerate(frames))      # a frame behind the cut: the control of the grain identity can differ
    assert S.windows_before(n, st.cuts, st.V, st.cuts[0]) == sum(1 for p in plan if p[0] < st.cuts[0])
    # every scene has a seam, and a window that keeps frames back
    assert all(any(p[3] for p in plan if a <= p[0] < b) for a, b in zip([0] + st.cuts, st.cuts + [n]))


def test_stack_d_runs_tiled_in_both_of_its_rectangles():
    st = S.STACKS["D"]()
    th, tw = st.kw["tile"]
    for rect in (st.rect, st.other_rect):
        hp, wp = windows.padded_size(rect[3], rect[2], "small")
        assert not windows.plan_tiles(hp, wp, th, tw, st.kw["tile_overlap"]).single


def payloads(fmt, h, w, seed, t=2):
    rng = np.random.default_rng(seed)
    c = R.constants(fmt)
    ch, cw = R.chroma_shape(fmt, h, w)
    return np.stack([R.join_planes(rng.integers(c["ylo"], c["yhi"] + 1, (h, w)), rng.integers(c["clo"], c["chi"] + 1, (ch, cw)),
                                   rng.integers(c["clo"], c["chi"] + 1, (ch, cw)), fmt) for _ in range(t)])


RECTS = [("D", S.F10, 48, 64, (6, 4, 52, 36)), ("D other", S.F10, 48, 64, (10, 8, 44, 32)), ("E", S.F10_444, 30, 44, (3, 5, 37, 21)),
         ("B", S.F8_LEFT, 48, 64, (8, 6, 48, 36))]


@pytest.mark.parametrize("name,fmt,h,w,rect", RECTS, ids=[r[0] for r in RECTS])
def test_grain_ref_with_a_rectangle_is_grain_ref_on_the_crop_pasted_back(name, fmt, h, w, rect):
    pay = payloads(fmt, h, w, 1)
    taps = grain.grain_taps(0.8)
    got = GR.grain_ref(pay, fmt, h, w, GR.BUMPY, taps, 0.5, 5, 3, rect=rect)
    inner = GR.grain_ref(P.crop_payloads(pay, fmt, h, w, rect), fmt, rect[3], rect[2], GR.BUMPY, taps, 0.5, 5, 3)
    assert np.array_equal(got, P.paste_payloads(pay, inner, fmt, h, w, rect)) and not np.array_equal(got, pay)


@pytest.mark.parametrize("name,fmt,h,w,rect", RECTS, ids=[r[0] for r in RECTS])
def test_diff_stats_ref_with_a_rectangle_is_diff_stats_ref_on_the_crops(name, fmt, h, w, rect):
    a, b = payloads(fmt, h, w, 2, t=3), payloads(fmt, h, w, 3, t=3)
    edge = 16 << (fmt.bits - 8)
    got = D.diff_stats_ref(a, b, fmt, h, w, rect=rect, edge=edge)
    crops = D.diff_stats_ref(P.crop_payloads(a, fmt, h, w, rect), P.crop_payloads(b, fmt, h, w, rect), fmt, rect[3], rect[2], edge=edge)
    assert np.array_equal(got, crops) and not np.array_equal(got, D.diff_stats_ref(a, b, fmt, h, w, edge=edge))


def test_the_input_as_written_is_the_payload_or_the_conversion_with_the_rectangle_converted_on_its_own():
    st = S.STACKS["B"]()
    assert all(np.array_equal(a, b) for a, b in zip(S.as_written(st, st.pay[:2], [st.rect] * 2), st.pay[:2]))
    st = S.STACKS["D"]()
    whole = S.converted(st.pay[:2], st.fmt, st.ofmt, st.h, st.w)
    got = S.as_written(st, st.pay[:2], [st.rect, None])
    assert np.array_equal(got[1], whole[1]) and not np.array_equal(got[0], whole[0])      # 4:2:0 chroma upsampled from the rectangle's own neighbours
    inner = S.converted(P.crop_payloads(np.stack(st.pay[:1]), st.fmt, st.h, st.w, st.rect), st.fmt, st.ofmt, st.rect[3], st.rect[2])
    assert np.array_equal(P.crop_payloads(got[0][None], st.ofmt, st.h, st.w, st.rect), inner)
    assert np.array_equal(P.paste_payloads(got[0][None], P.crop_payloads(whole[:1], st.ofmt, st.h, st.w, st.rect), st.ofmt, st.h, st.w, st.rect)[0], whole[0])
