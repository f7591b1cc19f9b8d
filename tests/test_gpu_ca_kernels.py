"""-m gpu: the squeeze-excite MLP, the closed-form CALayer of the dense CAB, SkipUpSample's tail and the ingest (csrc/sn_conv.hip: ca_mlp_kernel,
cab_ca_part_kernel<bf16_t>, cab_ca_kernel<bf16_t>, upsample2_add_kernel, ingest_kernel) through the C ABI against float64 on the CPU, element by
element.

tests/test_gpu_parity.py sees a CAB's scale only through the CAB's bf16 output at 8e-3 of the peak, and the fold's test uses sn_ca_mlp AS its
reference.  Here every element of every `ca` is held to the contract of tests/ca_cases.py -- a function of the entry point's own operands -- on
three operand families per case (dense, impulse rows on the seams of the 16 x nsplit split, impulse pixels on the corners and the seams of the
lines' 16 x nseg split), with `scratch` pre-filled with NaN and `ca` between sentinels; sn_cab_ca_lines must reproduce sn_cab_ca bit for bit
from the four border lines alone, and sn_cab_ca must not notice an interior of NaN.  A chain check runs the CAB's first conv on the device
and holds sn_cab_ca to the contract on the device's own pool and mid, and to the CALayer of conv2(stored mid).  sn_upsample2_add: every
stored value a bf16 rounding of a value within 6 u sum |terms| of float64, one-hot inputs bit-exact.  sn_ingest: bit-exact against torch.
Measured ratios go to parity_report_ca.json in $SN_PARITY_REPORT_DIR (default: parity_out/ at the repository root).
"""
import json
import os

import numpy as np
import pytest
import torch

import ca_cases as CA

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = []
GUARD = 1024                        # sentinel elements before and after every output buffer
SENT = 7.0
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_ca.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lb():
    from shiftnet_amd import lib as L
    return L.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]]).float()
    return bool((g == fill).all()) if fill == fill else bool(torch.isnan(g).all())


def dv(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).contiguous().to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class CabDev:
    """device weights of a CAB case and one launcher for sn_cab_ca / sn_cab_ca_lines, T frames per launch"""

    def __init__(self, lb, case, wts):
        self.lb, self.case = lb, case
        self.w2, self.wa, self.wb = dv(wts["w2"]), dv(wts["wa"]), dv(wts["wb"])
        self.cr = wts["cr"]
        self.nscratch = lb.sn_cab_ca_scratch_floats(CA.T)
        assert self.nscratch == CA.T * CA.NS * 5 * 128

    def run(self, partial, mid, lines_len=None, nan_interior=False):
        """ca [F][cpad] (numpy fp32) of F frames, CA.T per launch (the last launch is filled up with frames from the start)"""
        c = self.case
        F = partial.shape[0]
        out = np.zeros((F, c.cpad), np.float32)
        for f0 in range(0, F, CA.T):
            idx = [(f0 + k) if f0 + k < F else (f0 + k) % F for k in range(CA.T)]
            p = dv(partial[idx])
            m = np.array(mid[idx], dtype=np.float32)
            if nan_interior:
                m[:, 1:c.h - 1, 1:c.w - 1] = NAN
            if lines_len:
                ln = np.full((CA.T, 4, lines_len, c.cs), NAN, np.float32)
                ln[:, 0, :c.w], ln[:, 1, :c.w], ln[:, 2, :c.h], ln[:, 3, :c.h] = m[:, 0], m[:, c.h - 1], m[:, :, 0], m[:, :, c.w - 1]
                m = ln
            md = dv(m, torch.bfloat16)
            sbuf, scratch = guarded((self.nscratch,), torch.float32, NAN)
            cbuf, ca = guarded((CA.T, c.cpad), torch.float32, SENT)
            args = (c.cs, c.c, self.cr, c.h, c.w, self.w2.data_ptr(), self.wa.data_ptr(), self.wb.data_ptr(), scratch.data_ptr(), ca.data_ptr(), CA.T, stream())
            if lines_len:
                rc = self.lb.sn_cab_ca_lines(p.data_ptr(), c.nblk, c.cpad, md.data_ptr(), lines_len, *args)
            else:
                rc = self.lb.sn_cab_ca(p.data_ptr(), c.nblk, c.cpad, md.data_ptr(), *args)
            assert rc == 0, (c.id, rc)
            torch.cuda.synchronize()
            assert guards_intact(cbuf, SENT) and guards_intact(sbuf, NAN), f"{c.id}: wrote outside ca or scratch"
            got = ca.cpu().numpy()
            assert np.isfinite(got).all() and (got != SENT).all(), f"{c.id}: ca not written everywhere"
            for k, f in enumerate(idx):
                if f0 + k < F:
                    out[f] = got[k]
        return out


def held(name, got, ref, c):
    """every element inside its bound, pad entries exactly 0; (max err / tol, mean err / tol)"""
    assert got.shape == ref["ca"].shape, (name, got.shape)
    assert (got[..., c:] == 0).all(), f"{name}: ca[c, cpad) not zero"
    e = np.abs(got[..., :c].astype(np.float64) - ref["ca"][..., :c]) / ref["tol"][..., :c]
    print(f"{name}: max err/tol {e.max():.3g}")
    if not (e <= 1.0).all():
        i = np.unravel_index(int(e.argmax()), e.shape)
        raise AssertionError(f"{name}: {int((e > 1).sum())} of {e.size} elements out of bound, max err/tol {e.max():.3g} at {i}: got {got[i]:.9g} "
                             f"ref {ref['ca'][i]:.9g} tol {ref['tol'][i]:.3g}")
    return float(e.max()), float(e.mean())


@pytest.mark.parametrize("case", CA.CAB_CASES, ids=[c.id for c in CA.CAB_CASES])
def test_cab_ca_against_float64(case, lb):
    c = case
    wts = CA.cab_weights(c.variant, c.pre)
    d = CabDev(lb, c, wts)
    rec = dict(test="sn_cab_ca", id=c.id, shape=[CA.T, c.h, c.w, c.c, c.cs, c.cpad, wts["cr"], c.nblk], families={})
    fams = {}
    fams["dense"] = CA.dense_operands(c)[:2]
    fams["dense+8"] = CA.dense_operands(c, offset=8.0)[:2]
    fams["rows"] = CA.impulse_row_operands(c)[:2]
    pp, pm, px = CA.impulse_pixel_operands(c)
    fams["pixels"] = (pp, pm)
    got = {}
    for name, (p, m) in fams.items():
        ref = CA.cab_ca_reference(c, wts, p, m)
        got[name] = d.run(p, m)
        mx, mean = held(f"{c.id}:{name}", got[name], ref, c.c)
        rec["families"][name] = dict(frames=int(p.shape[0]), max_err_over_tol=mx, mean_share_of_bound=mean)
    # the four border lines alone, in line buffers of both lengths with NaN beyond each line: bit for bit
    for name in ("dense", "dense+8", "pixels"):
        p, m = fams[name]
        for ll in (max(c.h, c.w), max(c.h, c.w) + 5):
            assert np.array_equal(bits(d.run(p, m, lines_len=ll)), bits(got[name])), f"{c.id}:{name}: sn_cab_ca_lines({ll}) differs from sn_cab_ca"
    # only border pixels are read
    for name in ("dense", "dense+8"):
        p, m = fams[name]
        assert np.array_equal(bits(d.run(p, m, nan_interior=True)), bits(got[name])), f"{c.id}:{name}: sn_cab_ca read an interior pixel"
    # an interior pixel leaves ca at its zero-input value
    kinds = [k for (_, _, k) in px]
    if "interior" in kinds:
        zero = d.run(np.zeros_like(pp[:1]), np.zeros_like(pm[:1]))
        assert np.array_equal(bits(got["pixels"][kinds.index("interior")]), bits(zero[0])), f"{c.id}: an interior pixel changed ca"
    REPORT.append(rec)


class MlpDev:
    def __init__(self, lb, case, wts):
        self.lb, self.case = lb, case
        self.wa, self.wb = dv(wts["wa"]), dv(wts["wb"])

    def run(self, partial, inv_hw, bad="word"):
        """(ca [F][cpad], the bad word after the last launch or None)"""
        c = self.case
        F = partial.shape[0]
        out = np.zeros((F, c.cpad), np.float32)
        flag = torch.zeros((1,), dtype=torch.int32, device=DEV) if bad == "word" else None
        for f0 in range(0, F, CA.T):
            idx = [(f0 + k) if f0 + k < F else (f0 + k) % F for k in range(CA.T)]
            p = dv(partial[idx])
            cbuf, ca = guarded((CA.T, c.cpad), torch.float32, SENT)
            rc = self.lb.sn_ca_mlp(p.data_ptr(), c.nblk, c.cpad, c.c, c.cr, float(inv_hw), self.wa.data_ptr(), self.wb.data_ptr(), ca.data_ptr(), CA.T,
                                   None if flag is None else flag.data_ptr(), stream())
            assert rc == 0, (c.id, rc)
            torch.cuda.synchronize()
            assert guards_intact(cbuf, SENT), f"{c.id}: wrote outside ca"
            got = ca.cpu().numpy()
            for k, f in enumerate(idx):
                if f0 + k < F:
                    out[f] = got[k]
        return out, (None if flag is None else int(flag.item()))


@pytest.mark.parametrize("case", CA.MLP_CASES, ids=[c.id for c in CA.MLP_CASES])
def test_ca_mlp_against_float64(case, lb):
    c = case
    wts = CA.mlp_weights(c)
    d = MlpDev(lb, c, wts)
    rec = dict(test="sn_ca_mlp", id=c.id, shape=[CA.T, c.c, c.cpad, c.cr, c.nblk], families={})
    p, inv, _ = CA.mlp_operands(c)
    pi, _, _ = CA.mlp_impulse_operands(c)
    for name, part in (("dense", p), ("rows", pi)):
        got, bad = d.run(part, inv)
        assert np.isfinite(got).all() and (got != SENT).all(), f"{c.id}:{name}: ca not written everywhere"
        assert bad == 0, f"{c.id}:{name}: the bad word was raised on finite input"
        mx, mean = held(f"{c.id}:{name}", got, CA.ca_mlp_reference(c, wts, part, inv), c.c)
        rec["families"][name] = dict(frames=int(part.shape[0]), max_err_over_tol=mx, mean_share_of_bound=mean)
        got2, _ = d.run(part, inv, bad=None)                      # bad = NULL is accepted and changes nothing
        assert np.array_equal(bits(got2), bits(got)), f"{c.id}:{name}: bad = NULL changed ca"
    REPORT.append(rec)


@pytest.mark.parametrize("what", ["+inf", "-inf", "nan", "overflow"])
@pytest.mark.parametrize("cid", ["mlp14of16_b64", "mlp80of80_b1000", "mlp126of128_b9"])
def test_ca_mlp_bad_word(cid, what, lb):
    """a non-finite channel sum in a LOGICAL channel of ONE frame raises the word: +-inf, NaN, and two finite rows whose fp32 sum overflows"""
    c = next(k for k in CA.MLP_CASES if k.id == cid)
    wts = CA.mlp_weights(c)
    p, inv, _ = CA.mlp_operands(c)
    p = p.copy()
    ch, b = c.c - 1, c.nblk - 1
    if what == "overflow":
        p[1, 0, ch] = p[1, b, ch] = 3.0e38                        # rows 0 and nblk - 1: different threads for nblk > nsplit, the same one otherwise
    else:
        p[1, b, ch] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[what]
    assert np.isfinite(p).all() or what != "overflow"
    _, bad = MlpDev(lb, c, wts).run(p, inv)
    assert bad == 1, (cid, what, bad)
    REPORT.append(dict(test="sn_ca_mlp_bad", id=cid, what=what, bad=bad))


def test_refusals(lb):
    """every condition the three wrappers test answers SN_EINVAL and leaves ca at its sentinel"""
    c = CA.cab_by_id("cab18_5x7_b5")
    wts = CA.cab_weights(c.variant, c.pre)
    cr = wts["cr"]
    p, m, _ = CA.dense_operands(c)
    pd, md = dv(p), dv(m, torch.bfloat16)
    w2, wa, wb = dv(wts["w2"]), dv(wts["wa"]), dv(wts["wb"])
    scratch = torch.full((lb.sn_cab_ca_scratch_floats(CA.T),), NAN, dtype=torch.float32, device=DEV)
    ll = max(c.h, c.w)
    lines = torch.zeros((CA.T, 4, ll, c.cs), dtype=torch.bfloat16, device=DEV)
    cbuf, ca = guarded((CA.T, c.cpad), torch.float32, SENT)
    good = dict(partial=pd.data_ptr(), nblk=c.nblk, cpad=c.cpad, mid=md.data_ptr(), cs=c.cs, c=c.c, cr=cr, h=c.h, w=c.w, w2=w2.data_ptr(),
                wa=wa.data_ptr(), wb=wb.data_ptr(), scratch=scratch.data_ptr(), ca=ca.data_ptr(), lines_len=ll)
    n = 0

    def cab(lines_form, **over):
        a = dict(good, **over)
        if lines_form:
            if "mid" not in over:
                a["mid"] = lines.data_ptr()
            return lb.sn_cab_ca_lines(a["partial"], a["nblk"], a["cpad"], a["mid"], a["lines_len"], a["cs"], a["c"], a["cr"], a["h"], a["w"], a["w2"],
                                      a["wa"], a["wb"], a["scratch"], a["ca"], CA.T, stream())
        return lb.sn_cab_ca(a["partial"], a["nblk"], a["cpad"], a["mid"], a["cs"], a["c"], a["cr"], a["h"], a["w"], a["w2"], a["wa"], a["wb"],
                            a["scratch"], a["ca"], CA.T, stream())
    bad_cab = [dict(partial=None), dict(mid=None), dict(w2=None), dict(wa=None), dict(wb=None), dict(scratch=None), dict(cpad=8), dict(cpad=15),
               dict(cpad=136), dict(cs=136, cpad=128), dict(cs=20), dict(cs=12), dict(c=c.cs + 1), dict(cs=40, c=33), dict(cr=0), dict(cr=129),
               dict(nblk=0), dict(nblk=-1), dict(h=1), dict(w=1), dict(h=0), dict(w=0)]
    for lines_form in (False, True):
        for over in bad_cab + ([dict(lines_len=ll - 1), dict(lines_len=0), dict(lines_len=-1)] if lines_form else []):
            assert cab(lines_form, **over) == CA.EINVAL, (lines_form, over)
            n += 1
        assert cab(lines_form, ca=None) == CA.EINVAL
    mc = next(k for k in CA.MLP_CASES if k.id == "mlp30of32_b33")
    mw = CA.mlp_weights(mc)
    mp, inv, _ = CA.mlp_operands(mc)
    mpd, mwa, mwb = dv(mp), dv(mw["wa"]), dv(mw["wb"])
    mbuf, mca = guarded((CA.T, mc.cpad), torch.float32, SENT)
    mgood = dict(partial=mpd.data_ptr(), nblk=mc.nblk, cpad=mc.cpad, c=mc.c, cr=mc.cr, wa=mwa.data_ptr(), wb=mwb.data_ptr(), ca=mca.data_ptr())

    def mlp(**over):
        a = dict(mgood, **over)
        return lb.sn_ca_mlp(a["partial"], a["nblk"], a["cpad"], a["c"], a["cr"], float(inv), a["wa"], a["wb"], a["ca"], CA.T, None, stream())
    for over in (dict(partial=None), dict(wa=None), dict(wb=None), dict(ca=None), dict(cpad=8), dict(cpad=15), dict(cpad=136), dict(c=mc.cpad + 1),
                 dict(cr=0), dict(cr=129), dict(nblk=0), dict(nblk=-1)):
        assert mlp(**over) == CA.EINVAL, over
        n += 1
    torch.cuda.synchronize()
    assert (cbuf == SENT).all() and (mbuf == SENT).all() and torch.isnan(scratch).all(), "a refused call wrote something"
    # the same buffers are accepted as they are
    assert cab(False) == 0 and cab(True) == 0 and mlp() == 0
    torch.cuda.synchronize()
    assert guards_intact(cbuf, SENT) and guards_intact(mbuf, SENT) and not (ca == SENT).any() and not (mca == SENT).any()
    REPORT.append(dict(test="refusals", refused=n))


def test_engine_cab_on_a_one_pixel_high_map_raises(lb):
    """sn_cab_ca refuses h < 2 (the closed form needs two distinct border rows), the fused form steps aside (Engine._cab_fused: h < 2), and
    Engine.cab turns the refusal into ShiftNetLibError -- loudly, never a wrong scale.  The network reaches such a map from a frame 4 pixels
    high (Shift-Net-s: the third TFR_UNet level) or 8 (Shift-Net+: stage 1's coarsest level); DESIGN 7 files it."""
    from shiftnet_amd import lib as L
    from shiftnet_amd.engine import Act, Engine
    pre = "feat_extract.1."
    eng = Engine(CA.light_plan("gshift_deblur2", (pre,), DEV))
    for (h, w) in ((1, 6), (6, 1)):
        x = torch.zeros((CA.T, h, w, 16), dtype=torch.bfloat16, device=DEV)
        with pytest.raises(L.ShiftNetLibError, match="sn_cab_ca"):
            eng.cab(pre, Act(x, 14))
        torch.cuda.synchronize()
    out = eng.cab(pre, Act(torch.zeros((CA.T, 2, 2, 16), dtype=torch.bfloat16, device=DEV), 14))       # the smallest map it takes
    torch.cuda.synchronize()
    assert out.dims == (CA.T, 2, 2, 16) and (out.t.float() == 0).all()


# ---- chain check: the CAB's first conv on the device, then sn_cab_ca on the device's own pool and mid -------------------------------------

CHAIN = [("gshift_deblur2", "stage1.skip_attn1.", 64), ("gshift_deblur1", "stage1.encoder_level1.", 80), ("gshift_deblur2", "feat_extract.1.", 14),
         ("gshift_deblur1", "feat_extract.1.", 24)]


@pytest.mark.parametrize("variant,pre,c", CHAIN, ids=[f"c{k[2]}" for k in CHAIN])
def test_chain_conv1_pool_then_cab_ca(variant, pre, c, lb):
    from shiftnet_amd.engine import Act, Engine
    eng = Engine(CA.light_plan(variant, (pre,), DEV))
    q = eng.P.cas[pre + "CA"]
    cs = int(eng.P.convs[pre + "body.0"]["cs_in"])
    h, w = 45, 70
    g = torch.Generator().manual_seed(4100 + c)
    x = torch.randn((CA.T, h, w, cs), generator=g) * torch.exp2(torch.rand((CA.T, 1, 1, cs), generator=g) * 6.0 - 3.0)
    x[..., c:] = 0.0
    slope = eng.P.scalar(pre + "body.1.weight")
    mid, pool, npix = eng.conv(pre + "body.0", [Act(x.to(torch.bfloat16).to(DEV), c)], prelu=slope, pool=True)
    _, nblk, cpad = pool.shape
    assert npix == h * w and mid.dims == (CA.T, h, w, cs)
    sbuf, scratch = guarded((lb.sn_cab_ca_scratch_floats(CA.T),), torch.float32, NAN)
    cbuf, ca = guarded((CA.T, cpad), torch.float32, SENT)
    rc = lb.sn_cab_ca(pool.data_ptr(), nblk, cpad, mid.t.data_ptr(), cs, q["c"], q["cr"], h, w, q["w2"].data_ptr(), q["wa"].data_ptr(),
                      q["wb"].data_ptr(), scratch.data_ptr(), ca.data_ptr(), CA.T, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(cbuf, SENT) and guards_intact(sbuf, NAN)
    case = CA.CabCase(f"chain{c}", variant, pre, c, cs, cpad, h, w, nblk, 0)
    wts = {"w2": q["w2"].cpu().numpy(), "wa": q["wa"].cpu().numpy(), "wb": q["wb"].cpu().numpy()}
    got = ca.cpu().numpy()
    pool_h, mid_h = pool.cpu().numpy(), mid.t.float().cpu().numpy()
    # (1) the contract on the device's own operands (the pool rows themselves are pinned by the conv test)
    mx, mean = held(f"chain{c}:contract", got, CA.cab_ca_reference(case, wts, pool_h, mid_h), c)
    # (2) the CALayer of conv2(stored mid): the pool sums conv1's fp32 accumulators, mid stores their bf16 roundings -- 2^-9 sum_p |mid| per channel
    one = CA.CabCase(f"chain{c}", variant, pre, c, cs, cpad, h, w, 1, 0)
    exact = np.zeros((CA.T, 1, cpad))
    exact[:, 0, :cs] = mid_h.astype(np.float64).sum((1, 2))
    extra = 2.0 ** -9 * np.abs(mid_h.astype(np.float64)).sum((1, 2))[:, :c]
    ref2 = CA.cab_ca_reference(case, wts, pool_h, mid_h, e_tot_extra=extra)
    only = CA.cab_ca_reference(one, wts, exact, mid_h, e_tot_extra=extra)["tol"] - CA.cab_ca_reference(one, wts, exact, mid_h)["tol"]
    want = np.zeros_like(ref2["ca"])
    want[:, :c] = CA.torch_calayer(case, wts, mid_h)
    assert np.abs(CA.cab_ca_reference(one, wts, exact, mid_h)["ca"] - want).max() <= 1e-10
    err = np.abs(got.astype(np.float64) - want)[:, :c]
    share, share_term = float((err / ref2["tol"][:, :c]).max()), float((err / only[:, :c]).max())
    print(f"chain{c}: err / (contract + 2^-9 term) {share:.3g}, err / the 2^-9 term alone {share_term:.3g}, max err {err.max():.3g}")
    assert share <= 1.0, (c, share)
    REPORT.append(dict(test="chain", id=f"chain{c}", shape=[CA.T, h, w, c, cs, cpad, int(q["cr"]), int(nblk)], contract_max_err_over_tol=mx,
                       contract_mean_share=mean, calayer_err_over_bound=share, calayer_err_over_rounding_term=share_term, calayer_max_err=float(err.max())))


# ---- sn_upsample2_add ----------------------------------------------------------------------------------------------------------------------

def run_upsample(lb, lo, res):
    T, hs, ws, cs = lo.shape
    lod, resd = lo.contiguous().to(DEV), res.contiguous().to(DEV)
    obuf, out = guarded((T, 2 * hs, 2 * ws, cs), torch.bfloat16, NAN)
    rc = lb.sn_upsample2_add(lod.data_ptr(), resd.data_ptr(), out.data_ptr(), T, hs, ws, cs, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(obuf, NAN), "wrote outside the output"
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"{int(np.isnan(got).sum())} elements not written"
    return got


@pytest.mark.parametrize("cs", CA.UP_CS)
@pytest.mark.parametrize("hw", CA.UP_MAPS, ids=[f"{h}x{w}" for h, w in CA.UP_MAPS])
def test_upsample2_add_against_float64(hw, cs, lb):
    hs, ws = hw
    lo, res = CA.upsample_operands(hs, ws, cs, seed=7000 + 100 * hs + ws + cs)
    got = run_upsample(lb, lo, res)
    ref, tol = CA.upsample_add_reference(lo.float().numpy(), res.float().numpy())
    a, b = CA.upsample_interval(ref, tol)
    outside = (got < a) | (got > b)
    assert not outside.any(), (f"{hs}x{ws}x{cs}: {int(outside.sum())} stored values are no bf16 rounding of a value within 6 u sum|terms| of ref; first: got "
                               f"{got[outside][0]:.9g} interval [{a[outside][0]:.9g}, {b[outside][0]:.9g}]")
    at_end = float(((got != CA.round_bf16_f64(ref))).mean())
    # one-hot inputs, power-of-two amplitudes (another one per channel, the second frame negated), res = 0: bit-exact
    amp = torch.exp2((torch.arange(cs) % 8 - 3).float())
    for (y, x) in CA.upsample_impulses(hs, ws):
        one = torch.zeros((CA.UP_T, hs, ws, cs))
        one[0, y, x], one[1, y, x] = amp, -2.0 * amp
        g1 = run_upsample(lb, one.to(torch.bfloat16), torch.zeros((CA.UP_T, 2 * hs, 2 * ws, cs), dtype=torch.bfloat16))
        r1, _ = CA.upsample_add_reference(one.numpy(), np.zeros((CA.UP_T, 2 * hs, 2 * ws, cs)))
        assert np.array_equal(g1, r1), f"{hs}x{ws}x{cs}: the footprint of pixel ({y}, {x}) is not exact"
    REPORT.append(dict(test="sn_upsample2_add", id=f"{hs}x{ws}x{cs}", shape=[CA.UP_T, hs, ws, cs], outside=0, share_not_the_rounding_of_ref=at_end))


def test_upsample2_add_refusals(lb):
    lo, res = CA.upsample_operands(2, 2, 16, seed=1)
    lod, resd = lo.to(DEV), res.to(DEV)
    obuf, out = guarded((CA.UP_T, 4, 4, 16), torch.bfloat16, SENT)
    st = stream()
    assert lb.sn_upsample2_add(lod.data_ptr(), resd.data_ptr(), out.data_ptr(), CA.UP_T, 2, 2, 12, st) == CA.EINVAL
    assert lb.sn_upsample2_add(lod.data_ptr(), resd.data_ptr(), out.data_ptr(), CA.UP_T, 2, 2, 0, st) == CA.EINVAL
    assert lb.sn_upsample2_add(None, resd.data_ptr(), out.data_ptr(), CA.UP_T, 2, 2, 16, st) == CA.EINVAL
    assert lb.sn_upsample2_add(lod.data_ptr(), None, out.data_ptr(), CA.UP_T, 2, 2, 16, st) == CA.EINVAL
    assert lb.sn_upsample2_add(lod.data_ptr(), resd.data_ptr(), None, CA.UP_T, 2, 2, 16, st) == CA.EINVAL
    for (T, hs, ws) in ((0, 2, 2), (CA.UP_T, 0, 2), (CA.UP_T, 2, 0)):
        assert lb.sn_upsample2_add(lod.data_ptr(), resd.data_ptr(), out.data_ptr(), T, hs, ws, 16, st) == CA.EINVAL
    torch.cuda.synchronize()
    assert (obuf.float() == SENT).all()


# ---- sn_ingest -----------------------------------------------------------------------------------------------------------------------------

DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


@pytest.mark.parametrize("C", range(1, 9))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_ingest_bit_exact(dtype, C, lb):
    """C = 1 .. 7 with a noise plane (lane C), C = 8 without one; lanes above the logical channels are +0"""
    for HW, (H, W) in zip(CA.INGEST_HW, ((1, 1), (5, 51), (1, 257))):
        src, nz = CA.ingest_operands(dtype, C, HW, C < 8, seed=8000 + 10 * C + HW)
        ref = CA.ingest_reference(src, nz)
        sd, nd = src.to(DEV), (None if nz is None else nz.to(DEV))
        dbuf, dst = guarded((CA.INGEST_T, HW, 8), torch.bfloat16, NAN)
        rc = lb.sn_ingest(sd.data_ptr(), DT[dtype], None if nd is None else nd.data_ptr(), dst.data_ptr(), CA.INGEST_T, C, H, W, stream())
        assert rc == 0, (dtype, C, HW, rc)
        torch.cuda.synchronize()
        assert guards_intact(dbuf, NAN), (dtype, C, HW)
        got = dst.cpu()
        assert not torch.isnan(got.float()).any(), (dtype, C, HW, "not written everywhere")
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (dtype, C, HW)
        n = C + (1 if nz is not None else 0)
        assert (got[..., n:].view(torch.int16) == 0).all()
    REPORT.append(dict(test="sn_ingest", id=f"{DT[dtype]}_{C}", bit_exact=True))


def test_ingest_refusals(lb):
    src, nz = CA.ingest_operands(torch.float32, 8, 255, False, seed=3)
    _, nz = CA.ingest_operands(torch.float32, 1, 255, True, seed=4)
    sd, nd = src.to(DEV), nz.to(DEV)
    dbuf, dst = guarded((CA.INGEST_T, 255, 8), torch.bfloat16, SENT)
    st = stream()
    assert lb.sn_ingest(sd.data_ptr(), 0, nd.data_ptr(), dst.data_ptr(), CA.INGEST_T, 8, 5, 51, st) == CA.EINVAL      # C = 8 with a noise plane
    assert lb.sn_ingest(sd.data_ptr(), 0, None, dst.data_ptr(), CA.INGEST_T, 0, 5, 51, st) == CA.EINVAL
    assert lb.sn_ingest(sd.data_ptr(), 3, None, dst.data_ptr(), CA.INGEST_T, 3, 5, 51, st) == CA.EINVAL
    assert lb.sn_ingest(sd.data_ptr(), -1, None, dst.data_ptr(), CA.INGEST_T, 3, 5, 51, st) == CA.EINVAL
    assert lb.sn_ingest(None, 0, None, dst.data_ptr(), CA.INGEST_T, 3, 5, 51, st) == CA.EINVAL
    assert lb.sn_ingest(sd.data_ptr(), 0, None, None, CA.INGEST_T, 3, 5, 51, st) == CA.EINVAL
    torch.cuda.synchronize()
    assert (dbuf.float() == SENT).all()
