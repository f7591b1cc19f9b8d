"""-m gpu: the video restorer with as many options on at once as its refusals allow (the three stacks of tests/stack_cases.py), checked one option at
a time.  The docstring of ``VideoRestorer`` states its contract as identities between runs; every test below takes one of them and asserts it with
every other option of the stack still on: the run against the run with one option taken away, followed by that option's numpy restatement under
tests/.  Bytes, integer sums and the floats the host derives from them are compared with == (``repr`` where nan is legal).  Two exceptions, both
sums that the device forms in floating point: the SSIM tile sums and the NIQE sums are taken from the kernels through their bindings, as
tests/test_gpu_restorer_fullref.py and tests/test_gpu_restorer_niqe.py take them, and the restatement of the SSIM sums is held to
tests/test_gpu_ssim.py's SSIM_ATOL beside that.  Five identities have a control: a wrong rule, applied to outputs already
computed, must give other bytes or sums.  DESIGN.md 3.41 lists which identity runs on which stack."""
import numpy as np
import pytest
import torch

import blur_ref as BL
import degrade_ref as DG
import diff_stats_mv_ref as DM
import diff_stats_ref as D
import grain_ref as GR
import mix_ref as MX
import motion_ref as M
import niqe_ref as NR
import picture_ref as P
import ssim_ref as SR
import stack_cases as S
import test_gpu_restorer_sequence as Q
import tile_ref as TL
import time_ref as TR
import yuv_ref as R
from shiftnet_amd import fullref as F
from shiftnet_amd import grain, niqe, noise, restore, windows
from shiftnet_amd.io_edges import ingest_yuv, niqe_sums_yuv, noise_map_level, ssim_sums_yuv, yuv_fmt
from test_gpu_niqe import SCORE_RTOL
from test_gpu_restorer_niqe import same_pairs
from test_gpu_restorer_options import TIMING, same
from test_gpu_ssim import SSIM_ATOL

pytestmark = pytest.mark.gpu

calls = Q.calls                                                    # the recorder of the launch-order file
CUT_STATS = ("cut_measure", "thumb_frames", "thumb_launches", "cuts_ignored")
GRAIN_STATS = S.GRAIN_KEYS + ("window_grain", "grain_launches")
ALL, DENOISE = ["D", "E", "B"], ["D", "E"]


def records(stats, but=()):
    """The records of a run without the timers, every value as its ``repr``: exact for a float, and nan equals nan."""
    return {k: repr(v) for k, v in stats.items() if k not in TIMING and k not in but}


def lists(stats, but=()):
    """The per-window and per-frame records, which concatenate when a stream is restored scene by scene.  The two lists of report rows, which the host
    derives from the sums and which carry the frame's and the window's number in the stream, are left to the sums."""
    but = tuple(but) + ("frame_report", "frame_report_motion")
    return {k: v for k, v in stats.items() if isinstance(v, list) and k not in TIMING and k not in but
            and (k.startswith(("window_", "frame_")) or k in ("pair_sums_mv", "seam_rms"))}


def crop(frames, fmt, h, w, rect):
    return list(P.crop_payloads(np.stack(frames), fmt, h, w, rect))


def paste(full, inner, fmt, h, w, rect):
    return list(P.paste_payloads(np.stack(full), np.stack(inner), fmt, h, w, rect))


class World:
    """One stack: its network and its runs, each made once, when a test first asks, and left unchanged."""

    def __init__(self, name):
        self.st = st = S.STACKS[name]()
        self.net = restore.load_net(st.variant, "synthetic", st.dtype)
        self.memo = {}

    def run(self, pay=None, gt="own", drop=(), h=None, w=None, times=1, **over):
        """-> per restore() on one object (frames, stats, the payloads the stage in front handed on).  gt="own": the stack's truth while the report is on."""
        st = self.st
        kw = {k: v for k, v in st.kw.items() if k not in drop}
        kw.update(over)
        vr = restore.VideoRestorer(self.net, S.ONE_LEN, **kw)
        if gt == "own":
            gt = st.gt
        out = []
        for _ in range(times):
            seen, more = [], {}
            if gt is not None and kw.get("report"):
                more["gt"] = iter(gt)
            if kw.get("deflicker") is not None:
                more["deflickered"] = lambda p: seen.append(p.copy())
            elif kw.get("add_noise") is not None or kw.get("add_blur") is not None:
                more["degraded"] = lambda p: seen.append(p.copy())
            frames = list(vr.restore(iter(st.pay if pay is None else pay), yuv_fmt(*st.fmt), h or st.h, w or st.w, **more))
            out.append((frames, dict(vr.stats), seen))
        return out if times > 1 else out[0]

    def get(self, name):
        if name not in self.memo:
            self.memo[name] = getattr(self, "_" + name)()
        return self.memo[name]

    # -- the runs --------------------------------------------------------------------------------------------------------------------
    def _twice(self):
        return {p: self.run(times=2, pipeline=p) for p in (True, False)}

    def _full(self):
        return self.get("twice")[True][0]

    def _cuts(self):
        """The scene starts the full run used: the listed ones, or those it found."""
        return list(self.get("full")[1]["cuts"])

    def _maps(self):
        return S.frame_maps(len(self.st.pay), self.get("cuts"), self.st.V)

    def _rects(self):
        """Per written frame the rectangle of its window."""
        frames, _ = self.get("maps")
        return [self.get("full")[1]["window_picture"][k] for k, _ in frames]

    def _own(self):
        """The input as written of the full run."""
        return S.as_written(self.st, self.get("full")[2], self.get("rects"))

    def _no_grain(self):
        return self.run(drop=S.GRAIN_KEYS)

    def _no_report(self):
        return self.run(drop=S.REPORT_KEYS, gt=None)

    def _core(self):
        """Grain and report off: what the hand assembly of identity 9 has to write."""
        return self.run(drop=S.GRAIN_KEYS + S.REPORT_KEYS, gt=None) if "grain" in self.st.kw else self.get("full")

    def _truth(self):
        """The truth of the report: the stream given as ``gt``, or the clean frames under ``add_noise``."""
        return self.st.gt if self.st.gt is not None else self.st.pay

    def _behind_stage(self):
        """The stack without its front stage, fed the payloads that stage handed on; the clean frames are then the truth by hand."""
        return self.run(pay=self.get("full")[2], gt=self.get("truth"), drop=self.st.stage_keys)

    def _inner(self):
        """The stack on the cropped stream, behind the front stage (which sees the whole frame by design): the payloads handed on and the truth cropped
        to the rectangle, no picture, the cuts listed as the full run used them (the detector keeps looking at the whole frame)."""
        st, r = self.st, self.st.rect
        gt = crop(self.get("truth"), st.ofmt, st.h, st.w, r) if st.kw.get("report") else None
        return self.run(pay=crop(self.get("full")[2], st.fmt, st.h, st.w, r), gt=gt, drop=st.stage_keys + ("picture", "bar_level"), h=r[3], w=r[2],
                        scene_cuts=self.get("cuts"))

    def _windows(self):
        """The hand assembly's float32 result of every window, cross-faded with its predecessor's: (lo, written, the scene's start, the first input
        frame, the rectangle, float32 [written, 3, hp, wp]) per window, and the seams."""
        st, net = self.st, self.net
        _, stats, fed = self.get("full")
        f, dt = yuv_fmt(*st.fmt), next(net.parameters()).dtype
        lo_c, hi_c = noise.clip_codes(st.fmt.bits, st.fmt.range)
        w_old, w_new = TR.weights(st.V)
        out, seams, carry, held = [], [], None, None
        for k, (lo, cnt, idx, head, wr) in enumerate(TR.scene_plan(len(fed), S.ONE_LEN, self.get("cuts"), st.V)):
            rect = stats["window_picture"][k]
            h, w = (st.h, st.w) if rect is None else (rect[3], rect[2])
            hp, wp = windows.padded_size(h, w, net.V.topo)
            dev = torch.from_numpy(np.stack([fed[i] for i in idx])).cuda()
            x = ingest_yuv(dev, f, st.h, st.w, hp, wp, dt, rect=rect)
            x32 = ingest_yuv(dev, f, st.h, st.w, hp, wp, torch.float32, rect=rect) if dt != torch.float32 else None
            short = {} if x32 is None else {"shortcut": x32}
            nm = ()
            if net.V.denoise and "window_nlf" in stats:             # the plane of the window's curve, from the package's wrapper
                nm = (noise_map_level(dev, f, st.h, st.w, hp, wp, [c / 255.0 for c in stats["window_nlf"][k]], dt, lo_c, hi_c, rect=rect),)
            elif net.V.denoise:
                nm = (torch.full((1, 1, 1, 1, 1), stats["window_sigma"][k] / 255.0, dtype=dt, device="cuda").expand(1, len(idx), 1, hp, wp),)
            with torch.no_grad():
                if st.tiled:
                    plan = windows.plan_tiles(hp, wp, *st.kw["tile"], st.kw["tile_overlap"])
                    results = []
                    for y0, x0, th, tw in plan.tiles:              # contiguous crops in plan order
                        c = (slice(None), slice(None), slice(None), slice(y0, y0 + th), slice(x0, x0 + tw))
                        args = tuple(a[c].contiguous() for a in (x,) + nm)
                        results.append(net.forward_fp32_out(*args, shortcut=x32[c].contiguous()).cpu().numpy())
                    o = TL.blend(results, plan, (cnt, 3, hp, wp))
                else:
                    o = net.forward_ensemble_fp32_out(x, *nm, ensemble=st.kw["ensemble"], time=st.kw.get("ensemble_time", False), **short).cpu().numpy().copy()
            assert o.dtype == np.float32 and o.shape == (cnt, 3, hp, wp)
            if head and carry is not None and held == (rect,):
                seams.append([TR.seam_rms(row, h, w) for row in TR.seam_sq(carry, o[:st.V], h, w)])
                o[:st.V] = TR.crossfade(carry, o[:st.V], w_old, w_new)
            else:
                seams.append(None)
            carry, held = (o[cnt - st.V:].copy(), (rect,)) if wr < cnt else (None, None)
            scene = max([0] + [c for c in self.get("cuts") if c <= lo])
            out.append((lo, wr, scene, idx[0], rect, o[:wr].copy()))
        return out, seams

    def written(self, first_written=True):
        """The mixed, dithered egress of the hand assembly's windows by tests/mix_ref.py.  The dither is keyed by the number, in its scene, of the
        window's first WRITTEN frame; ``first_written=False`` is the control: the first frame the window is fed."""
        st, own, out = self.st, self.get("own"), []
        for lo, wr, scene, first_fed, rect, o in self.get("windows")[0]:
            key = (st.kw["dither_seed"], (lo if first_written else first_fed) - scene)
            ref = np.stack(own[lo:lo + wr])
            if rect is None:
                out += list(MX.egress(o, st.ofmt, st.h, st.w, st.mix, ref, dither=key))
            else:
                inner = MX.egress(o, st.ofmt, rect[3], rect[2], st.mix, P.crop_payloads(ref, st.ofmt, st.h, st.w, rect), dither=key)
                out += list(P.paste_payloads(ref, inner, st.ofmt, st.h, st.w, rect))
        return out


WORLDS = {}


@pytest.fixture(scope="module")
def world(request):
    if request.param not in WORLDS:
        WORLDS[request.param] = World(request.param)
    return WORLDS[request.param]


def stacks(names):
    return pytest.mark.parametrize("world", names, indirect=True)


def grained(wd, base, stats, per_scene=True):
    """``base`` with the restatement's grain, frame by frame: the knots of the frame's window, the frame's number in its scene (``per_scene=False``, the
    control: in the stream), the window's rectangle, the format written."""
    st = wd.st
    taps, out = grain.grain_taps(st.kw["grain_size"]), []
    for i, ((k, number), p) in enumerate(zip(wd.get("maps")[0], base)):
        out.append(GR.grain_ref(p[None], st.ofmt, st.h, st.w, stats["window_grain"][k], taps, st.kw["grain_chroma"], st.kw["grain_seed"],
                                number if per_scene else i, rect=stats["window_picture"][k])[0])
    return out


# ---- 1: pipeline and repeat -----------------------------------------------------------------------------------------------------------------
@stacks(ALL)
def test_01_the_pipeline_changes_nothing_and_a_second_restore_repeats_the_first(world):
    st, got = world.st, world.get("twice")
    (piped, pstats, pseen), (serial, sstats, sseen) = got[True][0], got[False][0]
    assert len(piped) == len(st.pay) == pstats["frames"] and all(p.size == R.frame_bytes(st.ofmt, st.h, st.w) for p in piped)
    assert same(piped, serial) and same(pseen, sseen) and records(pstats) == records(sstats) and set(pstats) == set(sstats)
    for p in (True, False):
        (first, fstats, fseen), (second, sstats, sseen) = got[p]
        assert same(first, second) and same(fseen, sseen) and records(fstats) == records(sstats) and set(fstats) == set(sstats)
    # every option of the stack is on and recorded
    plan = TR.scene_plan(len(st.pay), S.ONE_LEN, st.cuts, st.V)
    assert pstats["cuts"] == st.cuts and pstats["windows"] == len(plan) and pstats["window_written"] == [p[4] for p in plan]
    assert pstats["window_picture"] == [st.rect] * len(plan) and pstats["window_overlap"] == st.V and pstats["dither"] == "tpdf"
    assert all(s is not None for s, p in zip(pstats["seam_rms"], plan) if p[3]) and all(k in pstats for k in st.stage_stats)
    if st.name == "D":
        assert pstats["out_format"] == "420p10" and pstats["amount"] == (0.7, 0.4) and all(len(t) == 12 for t in pstats["window_tiles"])
        assert pstats["sigma_motion"] == "blocks" and pstats["grain"] == "auto:0.5" and len(pstats["frame_fullref"]) == len(st.pay)
        assert all(max(curve) > min(curve) > 0.0 for curve in pstats["window_nlf"])      # every window has a curve of its own, not the filler of no estimate
    if st.name == "E":
        assert len(pstats["ensemble_members"]) == 8 and pstats["sigma_estimator"] == "temporal" and len(pstats["frame_fullref"]) == len(st.pay)
        assert all(np.isfinite(v) for pair in pstats["frame_niqe"] for v in pair)      # the grown picture has its two blocks
    if st.name == "B":
        assert pstats["view"] == "removed" and pstats["ensemble_members"] == [0, 1] and pstats["blur_launches"] > 0


# ---- 2: grain -------------------------------------------------------------------------------------------------------------------------------
@stacks(DENOISE)
def test_02_the_run_is_the_run_without_grain_then_the_restatement_frame_by_frame(world):
    st = world.st
    got, stats, _ = world.get("full")
    base, bstats, _ = world.get("no_grain")
    assert same(got, grained(world, base, stats)) and not same(got, base)
    assert not any(k in bstats for k in GRAIN_STATS) and stats["grain_launches"] == stats["windows"]
    assert {k: v for k, v in lists(stats).items() if k in ("window_sigma", "window_nlf", "window_picture", "seam_rms", "window_written")} == \
        {k: v for k, v in lists(bstats).items() if k in ("window_sigma", "window_nlf", "window_picture", "seam_rms", "window_written")}
    if st.name == "D":                                             # "auto:0.5": half of the curve every window was restored with
        assert stats["window_grain"] == [[0.5 * c for c in curve] for curve in stats["window_nlf"]]
    else:
        assert stats["window_grain"] == [S.GRAIN_CURVE] * stats["windows"]
    # control: the frame's number counted from the stream's start differs behind the cut, and only there
    wrong, cut = grained(world, base, stats, per_scene=False), world.get("cuts")[0]
    assert same(wrong[:cut], got[:cut]) and all(not np.array_equal(a, b) for a, b in zip(wrong[cut:], got[cut:]))


# ---- 3: the report --------------------------------------------------------------------------------------------------------------------------
@stacks(DENOISE)
def test_03_the_report_changes_no_byte_and_its_sums_are_the_restatements_on_what_was_written(world):
    st = world.st
    got, stats, _ = world.get("full")
    off, ostats, _ = world.get("no_report")
    assert same(got, off) and not any(k.startswith(("frame_", "report", "pair_sums", "fullref")) for k in ostats if k != "frame_deflicker")
    own, truth, of = world.get("own"), world.get("truth"), yuv_fmt(*st.ofmt)
    edge = 16 << (st.ofmt.bits - 8)
    mu, cov, win7 = niqe.load_params(niqe.default_params_path())
    taps = torch.from_numpy(win7.astype(np.float32)).cuda()
    sums, pairs, full_refs, by_ssim_ref, scores, by_niqe_ref = [], [], [], [], [], []
    for k, (lo, wr, _) in enumerate(world.get("maps")[1]):
        rect = stats["window_picture"][k]
        h, w = (st.h, st.w) if rect is None else (rect[3], rect[2])
        a, b, g = (np.stack(x[lo:lo + wr]) for x in (own, got, truth))
        sums += [[int(v) for v in r] for r in D.diff_stats_ref(a, b, st.ofmt, st.h, st.w, rect=rect, edge=edge)]
        if wr >= 2:                                                # along the vectors of the frames yielded; a window's last frame has no pair
            mv, _ = M.block_motion_ref(b, st.ofmt, st.h, st.w, rect=rect)
            pairs += [[int(v) for v in r] for r in DM.diff_stats_mv_ref(a, b, mv, st.ofmt, st.h, st.w, rect=rect)]
        pairs.append(None)
        si, so = (D.diff_stats_ref(g, x, st.ofmt, st.h, st.w, rect=rect, edge=0) for x in (a, b))
        dg, da, db = (torch.from_numpy(x).cuda() for x in (g, a, b))
        ti, to = (ssim_sums_yuv(dg, x, of, st.h, st.w, rect=rect).cpu().numpy() for x in (da, db))
        ri, ro = (SR.ssim_sums_ref(g, x, st.ofmt, st.h, st.w, rect) for x in (a, b))
        full_refs += [F.frame_fullref(si[i], so[i], ti[i], to[i], st.ofmt.bits, h, w) for i in range(wr)]
        by_ssim_ref += [F.frame_fullref(si[i], so[i], ri[i], ro[i], st.ofmt.bits, h, w) for i in range(wr)]
        if (h // 96) * (w // 96):
            ni, no = (niqe_sums_yuv(x, of, st.h, st.w, taps, rect=rect).cpu().numpy() for x in (da, db))
            scores += [(niqe.frame_score(ni[i], mu, cov), niqe.frame_score(no[i], mu, cov)) for i in range(wr)]
            # ... and from the plain long-double restatement of the sums, with the model's unrounded taps, on the same payloads
            pi, po = (NR.niqe_sums_ref(x, st.ofmt, st.h, st.w, win7, rect=rect, sums=NR.plain_sums_of_luma) for x in (a, b))
            by_niqe_ref += [(niqe.frame_score(pi[i], mu, cov), niqe.frame_score(po[i], mu, cov)) for i in range(wr)]
        else:                                                      # a picture without a whole 96 x 96 block has no score
            scores += [(float("nan"), float("nan"))] * wr
    assert stats["frame_sums"] == sums and stats["report_launches"] == stats["windows"]
    assert stats["pair_sums_mv"] == pairs and any(p is not None for p in pairs)
    assert stats["frame_fullref"] == full_refs and stats["fullref_launches"] == 4 * stats["windows"]
    worst = max(abs(a - b) for x, y in zip(full_refs, by_ssim_ref) for a, b in ((x.ssim_in, y.ssim_in), (x.ssim_out, y.ssim_out)))
    print(f"{st.name}: SSIM from the kernel's tile sums against the restatement's, largest difference {worst:.3g}")
    assert worst <= SSIM_ATOL
    assert same_pairs(stats["frame_niqe"], scores) and len(scores) == len(got)
    if st.name == "E":                                             # D's 36 x 52 picture holds no block: its scores are nan by construction
        assert len(by_niqe_ref) == len(got)
        worst = max(abs(a - b) / b for x, y in zip(stats["frame_niqe"], by_niqe_ref) for a, b in zip(x, y))
        print(f"{st.name}: NIQE against the score of the restatement's sums, largest relative difference {worst:.3g}")
        assert worst <= SCORE_RTOL
    else:
        assert by_niqe_ref == [] and all(np.isnan(v) for pair in stats["frame_niqe"] for v in pair)
    # control: the sums describe the stream with the grain, not the frames before it
    base = world.get("no_grain")[0]
    before = []
    for k, (lo, wr, _) in enumerate(world.get("maps")[1]):
        before += [[int(v) for v in r] for r in D.diff_stats_ref(np.stack(own[lo:lo + wr]), np.stack(base[lo:lo + wr]), st.ofmt, st.h, st.w,
                                                                  rect=stats["window_picture"][k], edge=edge)]
    assert all(a != b for a, b in zip(before, sums))


# ---- 4: the front stages --------------------------------------------------------------------------------------------------------------------
@stacks(ALL)
def test_04_the_front_stage_hands_on_the_restatements_payloads_and_the_rest_runs_as_if_fed_them(world):
    st = world.st
    got, stats, seen = world.get("full")
    clean, cut = st.pay, st.cuts[0]
    if st.stage == "deflicker":                                    # clamped to the listed scenes
        want, info = S.deflickered_ref(clean, st.fmt, st.h, st.w, st.kw["deflicker"], cuts=st.cuts)
        assert stats["frame_deflicker"] == info
    elif st.stage == "add_noise":                                  # the frame index counted in the stream
        want = list(DG.degrade_ref(np.stack(clean), st.fmt, st.h, st.w, st.kw["add_noise"], st.kw["add_noise_seed"], 0))
        per_scene = DG.degrade_ref(np.stack(clean[cut:]), st.fmt, st.h, st.w, st.kw["add_noise"], st.kw["add_noise_seed"], 0)
        assert all(not np.array_equal(a, b) for a, b in zip(per_scene, seen[cut:]))      # control: the index counted in the scene
    else:                                                          # clamped to the listed scenes, the index counted in the stream
        want = list(BL.blur_stream(clean, st.fmt, st.h, st.w, st.kw["add_blur"], 2.2, cuts=st.cuts))
        # control: the right centre, the window clamped to the stream and not to the scene: other bytes on the frames whose window reaches across
        # the cut, and on those only
        across, r = BL.blur_stream(clean, st.fmt, st.h, st.w, st.kw["add_blur"], 2.2), st.kw["add_blur"] // 2
        differ = [f for f in range(len(clean)) if not np.array_equal(across[f], seen[f])]
        assert differ == list(range(cut - r, cut + r))
    assert len(seen) == len(clean) and same(seen, want) and not same(seen, clean)
    plain, pstats, _ = world.get("behind_stage")
    assert same(got, plain)
    assert records(stats, but=st.stage_stats) == records(pstats) and not any(k in pstats for k in st.stage_stats)


@stacks(["E", "B"])
def test_04b_the_refusals_that_need_a_stream(world):
    st = world.st
    f = yuv_fmt(*st.fmt)
    kw = dict(st.kw, report=True)                                  # B: the report in the place of the view, which excludes it
    kw.pop("view", None), kw.pop("removed_gain", None)
    with pytest.raises(ValueError, match=st.stage + r".*gt"):
        list(restore.VideoRestorer(world.net, S.ONE_LEN, **kw).restore(iter(st.pay), f, st.h, st.w, gt=iter(st.pay)))
    with pytest.raises(ValueError, match=st.stage + r".*report.*out_format"):
        list(restore.VideoRestorer(world.net, S.ONE_LEN, **dict(kw, out_format="420p10")).restore(iter(st.pay), f, st.h, st.w))
    # without the report another format out is fine for the stage: nothing needs the truth
    kw = {k: v for k, v in dict(kw, out_format="420p10").items() if k not in S.REPORT_KEYS + S.GRAIN_KEYS}
    assert len(list(restore.VideoRestorer(world.net, S.ONE_LEN, **kw).restore(iter(st.pay), f, st.h, st.w))) == len(st.pay)


# ---- 5: scenes ------------------------------------------------------------------------------------------------------------------------------
def scene_by_scene(world, pictures=None):
    """The runs on each scene's slice, concatenated: frames, the per-window and per-frame records, the payloads handed on."""
    st = world.st
    n, cut = len(st.pay), st.cuts[0]
    before = S.windows_before(n, st.cuts, st.V, cut)
    frames, recs, fed = [], {}, []
    for a, b, wa, wb in ((0, cut, 0, before), (cut, n, before, None)):
        over = {} if pictures is None else {"picture": pictures[wa:wb]}
        out, stats, seen = world.run(pay=st.pay[a:b], gt=None if st.gt is None else st.gt[a:b], drop=("scene_cuts",), **over)
        frames += out
        fed += seen
        for k, v in lists(stats).items():
            recs[k] = recs.get(k, []) + v
    return frames, recs, fed


@stacks(["D", "B"])
def test_05_listed_cuts_give_the_runs_on_each_scenes_slice_concatenated(world):
    st = world.st
    got, stats, seen = world.get("full")
    frames, recs, fed = scene_by_scene(world)
    assert same(got, frames) and same(seen, fed)
    assert records(lists(stats)) == records(recs)
    # the rectangle changes at the cut
    before = S.windows_before(len(st.pay), st.cuts, st.V, st.cuts[0])
    pictures = [st.rect] * before + [st.other_rect] * (stats["windows"] - before)
    got, stats, seen = world.run(picture=pictures)
    frames, recs, fed = scene_by_scene(world, pictures)
    assert stats["window_picture"] == pictures and same(got, frames) and same(seen, fed) and records(lists(stats)) == records(recs)
    assert not same(got, world.get("full")[0])


@stacks(["E"])
def test_05_found_cuts_give_the_run_with_those_cuts_listed(world):
    st = world.st
    got, stats, seen = world.get("full")
    assert stats["cuts"] == st.cuts                                 # the detector found the one cut of the clip
    listed, lstats, lseen = world.run(scene_cuts=list(stats["cuts"]))
    assert same(got, listed) and same(seen, lseen) and records(stats, but=CUT_STATS) == records(lstats, but=CUT_STATS)
    before = S.windows_before(len(st.pay), st.cuts, st.V, st.cuts[0])
    pictures = [st.rect] * before + [st.other_rect] * (stats["windows"] - before)
    got, stats, _ = world.run(picture=pictures)
    listed, lstats, _ = world.run(picture=pictures, scene_cuts=list(stats["cuts"]))
    assert stats["window_picture"] == pictures and stats["cuts"] == st.cuts
    assert same(got, listed) and records(stats, but=CUT_STATS) == records(lstats, but=CUT_STATS) and not same(got, world.get("full")[0])


# ---- 6: the picture -------------------------------------------------------------------------------------------------------------------------
@stacks(ALL)
def test_06_inside_the_rectangle_the_run_is_the_run_on_the_cropped_stream_and_outside_the_input_as_written(world):
    st, r = world.st, world.st.rect
    got, stats, seen = world.get("full")
    inner, istats, _ = world.get("inner")
    assert stats["window_picture"] == [r] * stats["windows"]       # E: found, window by window, under the noised bars
    inside = crop(got, st.ofmt, st.h, st.w, r)
    assert same(inside, inner)
    mine, theirs = lists(stats, but=st.stage_stats + ("window_picture",)), lists(istats, but=("window_picture",))
    assert records(mine) == records(theirs) and set(mine) >= {"window_written", "seam_rms"}
    if st.name != "B":                                             # every per-window estimate and every sum of the report
        assert {"window_sigma", "window_frame_sigma", "window_pair_sigma", "window_grain", "frame_sums", "pair_sums_mv", "frame_fullref", "frame_niqe"} <= set(mine)
    # outside: what the stage handed on (B, E), or that frame converted and undithered (D); grain and dither do not reach there
    outside = list(S.converted(seen, st.fmt, st.ofmt, st.h, st.w)) if st.ofmt != st.fmt else seen
    assert same(paste(got, crop(outside, st.ofmt, st.h, st.w, r), st.ofmt, st.h, st.w, r), outside)
    # control: the crop moved by two samples is another stream
    moved = (r[0], r[1] + 2, r[2], r[3])
    assert all(not np.array_equal(a, b) for a, b in zip(crop(got, st.ofmt, st.h, st.w, moved), inner))


# ---- 7: levels read back --------------------------------------------------------------------------------------------------------------------
@stacks(DENOISE)
def test_07_the_levels_a_run_reports_reproduce_its_bytes_when_listed(world):
    st = world.st
    got, stats, _ = world.get("full")
    if st.name == "D":      # "auto" scales what a window was restored with: the grain is given by hand, per identity 2, with the knots the run reported
        back, bstats, _ = world.run(sigma=list(stats["window_sigma"]), noise_model=[list(c) for c in stats["window_nlf"]],
                                    drop=("sigma_estimator", "sigma_motion") + S.GRAIN_KEYS)
        assert bstats["window_nlf"] == stats["window_nlf"] and bstats["nlf_launches"] == 0
        back = grained(world, back, stats)
    else:
        back, bstats, _ = world.run(sigma=list(stats["window_sigma"]), drop=("sigma_estimator",))
        assert bstats["frame_sums"] == stats["frame_sums"] and bstats["window_grain"] == stats["window_grain"]
    assert bstats["window_sigma"] == stats["window_sigma"] and "window_frame_sigma" not in bstats and bstats["seam_rms"] == stats["seam_rms"]
    assert same(got, back)


# ---- 8: amount 0 ----------------------------------------------------------------------------------------------------------------------------
@stacks(DENOISE)
def test_08_amount_zero_returns_the_input_as_written_byte_for_byte(world):
    zero, stats, seen = world.run(amount=0, drop=S.GRAIN_KEYS)
    assert stats["amount"] == (0.0, 0.0) and same(seen, world.get("full")[2])
    assert same(zero, world.get("own")) and not same(zero, world.get("core")[0])
    assert all(row[1] == row[2] == 0 and row[11] == row[12] == row[13] == row[14] == 0 for row in stats["frame_sums"])      # the report reads no change


# ---- 9: the core by hand --------------------------------------------------------------------------------------------------------------------
@stacks(ALL)
def test_09_the_core_is_the_hand_assembly_window_by_window(world):
    core, stats, _ = world.get("core")
    _, seams = world.get("windows")
    assert stats["seam_rms"] == seams and sum(s is not None for s in seams) == 2
    assert same(core, world.written())
    # control: keyed by the first frame the window is fed rather than by the first it writes, the dither is another on every frame
    assert all(not np.array_equal(a, b) for a, b in zip(core, world.written(first_written=False)))


# ---- 10: the launch order -------------------------------------------------------------------------------------------------------------------
@stacks(DENOISE)
def test_10_every_window_launches_crossfade_egress_grain_report_in_that_order(world, calls, monkeypatch):
    """D: tiles, a converted format and a truth stream; its 36 x 52 picture holds no NIQE block, so its windows launch no NIQE sums.  E: the ensemble,
    the truth from the stage in front, and a picture of two blocks: there the two NIQE launches sit between the motion pair and the truth's four."""
    st = world.st
    monkeypatch.setattr(Q, "OWN", Q.OWN + ("sn_geo_", "sn_time_", "sn_tile_"))
    vr = restore.VideoRestorer(world.net, S.ONE_LEN, pipeline=False, **st.kw)
    it = vr.restore(iter(st.pay), yuv_fmt(*st.fmt), st.h, st.w, **({} if st.gt is None else {"gt": iter(st.gt)}))
    plan = TR.scene_plan(len(st.pay), S.ONE_LEN, st.cuts, st.V)
    forward, members = ("sn_tile_accumulate", 12) if st.tiled else ("sn_geo_accumulate", 8)
    blocks = (st.rect[3] // 96) * (st.rect[2] // 96)
    assert (blocks > 0) == (st.name == "E")
    for lo, cnt, idx, head, wr in plan:                            # the serial driver hands a window's frames out before it stages the next
        del calls[:]
        for _ in range(wr):
            next(it)
        got = list(calls)
        tail = got[got.index("sn_time_crossfade"):] if head else got[got.index("sn_egress_yuv_mix"):]
        assert ("sn_time_crossfade" in got) == bool(head) and got.count("sn_time_crossfade") <= 1
        # the tiles or the members lie in front of the seam; as many again where the range guard tripped and they ran once more
        assert not any(c.startswith(("sn_tile_", "sn_geo_")) for c in tail) and got.count(forward) in (members, 2 * members)
        tail = [c for c in tail if not c.startswith(("sn_ingest_yuv", "sn_egress_yuv_rect")) and c != "sn_egress_yuv"]      # the input as written
        pairs = ["sn_yuv_block_motion", "sn_yuv_diff_stats_mv"] if wr >= 2 else []
        quality = ["sn_yuv_niqe_sums"] * 2 if blocks else []
        # the truth's two difference launches and two SSIM launches come last
        assert tail == (["sn_time_crossfade"] if head else []) + ["sn_egress_yuv_mix", "sn_yuv_grain", "sn_yuv_diff_stats"] + pairs + quality + \
            ["sn_yuv_diff_stats"] * 2 + ["sn_yuv_ssim_sums"] * 2
        assert got.count("sn_yuv_grain") == 1 and got.count("sn_yuv_diff_stats") == 3 and got.count("sn_egress_yuv_mix") == 1
    del calls[:]
    assert list(it) == [] and calls == []                          # nothing is launched behind the last frame
    assert vr.stats["grain_launches"] == vr.stats["report_launches"] == len(plan) and vr.stats["cuts"] == st.cuts
    assert vr.stats["report_quality_launches"] == (2 * len(plan) if blocks else 0)
