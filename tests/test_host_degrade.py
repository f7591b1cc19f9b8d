"""CPU tests of the added noise (shiftnet_amd/degrade.py, ``--add_noise``): the table, the field of samples as i.i.d. unit Gaussians, the project's own
noise estimator on clips degraded by the numpy restatement (tests/degrade_ref.py), the option's grammar, the refusals of the command line and of the C
entry point, and the new symbol.

Bounds.  The field's: five standard deviations of each estimator for N i.i.d. samples -- the mean's is 1 / sqrt(N), the variance's sqrt(2 / N), a
correlation coefficient's 1 / sqrt(N).  The estimator's: ``noise_ref.margin``, the project's own bound for injected noise."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import degrade_ref as DR
import noise_ref as N
import yuv_ref as R
from shiftnet_amd import degrade, restore_cli, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_table_has_mean_zero_unit_variance_and_is_antisymmetric():
    t = degrade.gauss_table()
    assert t.dtype == np.float32 and t.shape == (65536,) and not t.flags.writeable and degrade.gauss_table() is t
    t64 = t.astype(np.float64)
    assert math.fsum(t64) == 0.0
    assert np.array_equal(t, -t[::-1]) and np.all(np.diff(t) > 0)
    assert abs(math.fsum(t64 * t64) / 65536 - 1.0) <= 1e-6
    assert 4.3 < float(t[-1]) < 4.35                                # the tails end here
    # entry k is the quantile at (k + 0.5) / 65536 over the table's rms, stated on its own for three entries
    import statistics
    nd = statistics.NormalDist()
    q = [nd.inv_cdf((k + 0.5) / 65536) for k in range(65536)]
    rms = math.sqrt(math.fsum(v * v for v in q) / 65536)
    for k in (0, 40000, 65535):
        assert abs(float(t[k]) - q[k] / rms) <= 2.0 ** -24 * abs(q[k] / rms) * 1.01      # one float32 rounding


def corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(np.mean(a * b) / math.sqrt(np.mean(a * a) * np.mean(b * b)))


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_the_field_is_white_within_five_standard_deviations(seed):
    n = degrade.noise_field(seed, 0, 4, 128, 192)
    assert n.shape == (4, 3, 128, 192) and n.dtype == np.float32
    cnt = n.size
    mean, var = float(n.astype(np.float64).mean()), float(n.astype(np.float64).var())
    print(f"seed {seed}: mean {mean:.5f} (bound {5 / math.sqrt(cnt):.5f}), variance {var:.5f} (bound {5 * math.sqrt(2 / cnt):.5f})")
    assert abs(mean) <= 5 / math.sqrt(cnt) and abs(var - 1.0) <= 5 * math.sqrt(2 / cnt)
    pairs = {"right": (n[..., :-1], n[..., 1:]), "lower": (n[:, :, :-1], n[:, :, 1:]), "diagonal": (n[:, :, :-1, :-1], n[:, :, 1:, 1:]),
             "next frame": (n[:-1], n[1:]), "channel 0/1": (n[:, 0], n[:, 1]), "channel 1/2": (n[:, 1], n[:, 2]), "channel 0/2": (n[:, 0], n[:, 2])}
    for name, (a, b) in pairs.items():
        r = corr(a, b)
        print(f"seed {seed}: {name} {r:+.5f} (bound {5 / math.sqrt(a.size):.5f})")
        assert abs(r) <= 5 / math.sqrt(a.size), name
    # a pure function of the frame's number in the stream, and another field for another seed
    assert np.array_equal(degrade.noise_field(seed, 2, 2, 128, 192), n[2:])
    assert not np.array_equal(degrade.noise_field(seed + 1, 0, 1, 128, 192), n[:1])


CLEAN = {}


def clean_payloads(clip, fname, h=180, w=320, t=2):
    if (clip, fname) not in CLEAN:
        rgb = np.stack([N.CLIPS[clip](h, w)] * t).astype(np.float32)
        CLEAN[clip, fname] = R.egress_emu(rgb, N.FORMATS[fname], h, w)
    return CLEAN[clip, fname]


@pytest.mark.parametrize("fname", list(N.FORMATS))
@pytest.mark.parametrize("clip", list(N.CLIPS))
def test_the_estimator_reads_the_injected_sigma_within_the_projects_margin(clip, fname):
    h, w, fmt = 180, 320, N.FORMATS[fname]
    clean = clean_payloads(clip, fname)
    lo, hi = N.clip_codes(fmt)
    for s in (0, 2, 5, 10, 20, 30):
        p = DR.degrade_ref(clean, fmt, h, w, [float(s)] * 16, 7, 0)
        est = float(np.median([N.sigma_ref(hh, fmt) for hh in N.hist_ref(p, fmt, h, w, lo, hi)]))
        print(f"{clip} | {fname}: injected {s}, read {est:.3f} (margin {N.margin(s) if s else 0})")
        if s == 0:
            assert est == 0.0
        else:
            assert abs(est - s) <= N.margin(s)


def test_a_flat_curve_is_the_number_and_sigma_zero_is_the_round_trip():
    fmt = N.FORMATS["10-bit 709 limited 4:2:0"]
    clean = clean_payloads("smooth", "10-bit 709 limited 4:2:0")
    s = DR.sigma_plane(clean, fmt, 180, 320, [7.0] * 16)
    assert np.all(s == np.float32(7.0 / 255.0))
    fall = DR.sigma_plane(clean, fmt, 180, 320, DR.FALLING)
    assert fall.min() >= np.float32(1.5 / 255.0) and fall.max() <= np.float32(24.0 / 255.0) and fall.min() < fall.max()
    zero = DR.degrade_ref(clean, fmt, 180, 320, [0.0] * 16, 0, 0)
    assert np.array_equal(zero, R.egress_emu(R.ingest_emu(clean, fmt, 180, 320, 180, 320), fmt, 180, 320))


def test_parse_add_noise_and_the_restorers_form():
    assert degrade.parse_add_noise("10") == [10.0] * 16 and degrade.parse_add_noise("0") == [0.0] * 16 and degrade.parse_add_noise(" 2.5 ") == [2.5] * 16
    curve = [float(i) / 2 for i in range(16)]
    assert degrade.parse_add_noise(",".join(repr(v) for v in curve)) == curve
    for bad in ("", "ten", "-1", "nan", "inf", "1,2", ",".join(["1"] * 15), ",".join(["1"] * 17), ",".join(["1"] * 15 + ["-0.5"]), "1;2"):
        with pytest.raises(ValueError):
            degrade.parse_add_noise(bad)
    assert degrade.add_noise_form(None) == (None, 0) and degrade.add_noise_form(10, 3) == ([10.0] * 16, 3) and degrade.add_noise_form(curve, 2 ** 32 - 1) == (curve, 2 ** 32 - 1)
    for bad in (-1.0, float("nan"), [1.0] * 15, "10", True, [1.0] * 15 + [float("inf")]):
        with pytest.raises(ValueError, match="add_noise"):
            degrade.add_noise_form(bad)
    for bad in (-1, 2 ** 32, 0.5):
        with pytest.raises(ValueError, match="add_noise_seed"):
            degrade.add_noise_form(10.0, bad)


def _write(path, header, payloads):
    with open(path, "wb") as fh:
        wr = y4m.Y4MWriter(fh, header)
        for p in payloads:
            wr.write(p)


def test_the_command_line_takes_the_options_and_refuses_what_does_not_go_together(tmp_path, capsys):
    ap = restore_cli.make_parser()
    base = ["--variant", "denoise_small", "--checkpoint", "synthetic", "--sigma", "auto"]
    a = ap.parse_args(base + ["in.y4m", "out.y4m"])
    assert a.add_noise is None and a.add_noise_seed == 0 and a.degraded_out is None
    a = ap.parse_args(base + ["--add_noise", "10", "--add_noise_seed", "7", "--degraded_out", "d.y4m", "in.y4m", "out.y4m"])
    assert a.add_noise == [10.0] * 16 and a.add_noise_seed == 7 and a.degraded_out == "d.y4m"
    assert ap.parse_args(base + ["--add_noise", ",".join(str(i) for i in range(16)), "in.y4m", "out.y4m"]).add_noise == [float(i) for i in range(16)]
    for bad in ("-3", "1,2,3", "much"):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(base + ["--add_noise", bad, "in.y4m", "out.y4m"])
        assert e.value.code == 2 and "--add_noise" in capsys.readouterr().err
    # judged before any file is opened: the files named here do not exist
    gone = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]
    with pytest.raises(SystemExit) as e:
        restore_cli.main(base + ["--add_noise", "10", "--report", "/nonexistent/r.txt", "--gt", "/nonexistent/t.y4m"] + gone)
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--add_noise" in err and "--gt" in err
    for more in (["--add_noise_seed", "3"], ["--degraded_out", "/nonexistent/d.y4m"]):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + more + gone)
        assert e.value.code == 2 and "need --add_noise" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        restore_cli.main(base + ["--add_noise", "10", "--add_noise_seed", str(2 ** 32)] + gone)
    assert e.value.code == 2 and "--add_noise_seed" in capsys.readouterr().err
    # judged against the header of the stream read, before the network is loaded (no GPU here)
    hd = y4m.Y4MHeader(width=72, height=40, chroma="420jpeg")
    src = tmp_path / "in.y4m"
    _write(src, hd, [np.zeros(hd.frame_bytes, np.uint8)])
    with pytest.raises(SystemExit) as e:
        restore_cli.main(base + ["--add_noise", "10", "--report", str(tmp_path / "r.txt"), "--out_format", "444p10", str(src), str(tmp_path / "out.y4m")])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--add_noise" in err and "--out_format" in err and "C420jpeg" in err and "C444p10" in err


def test_header_build_list_and_library_have_the_new_symbol_and_the_entry_point_refuses_on_the_host():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_degrade.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_degrade.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    from shiftnet_amd.io_edges import yuv_fmt
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^typedef struct sn_yuv_degrade_noise \{ uint32_t seed; int t0; float knots\[16\]; \} sn_yuv_degrade_noise;", header, flags=re.M)
    assert re.search(r"^int sn_yuv_degrade\(const uint8_t\* src, const sn_yuv_fmt\* fmt, const sn_yuv_degrade_noise\* noise, const float\* gauss /\* device, 65536 \*/, "
                     r"uint8_t\* dst,\s+int T, int H, int W, void\* stream\);", header, flags=re.M)
    assert hasattr(lib, "sn_yuv_degrade") and "sn_yuv_degrade" in L.SYMBOLS and len(lib.sn_yuv_degrade.argtypes) == 9
    assert C.sizeof(L.YuvDegradeNoise) == 72 and [f[0] for f in L.YuvDegradeNoise._fields_] == ["seed", "t0", "knots"]
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    # the argument checks are host side and need no GPU: host memory is refused before anything would read it
    arr = np.zeros(1 << 20, np.uint8)
    buf = arr.ctypes.data + (-arr.ctypes.data) % 16
    src, dst, gauss = buf, buf + (1 << 18), buf + (1 << 19)                  # 40 x 72 x 3 samples x 2 bytes x 2 frames < 2^18
    f8, f10 = yuv_fmt(8, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED), yuv_fmt(10, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED)

    def noise(t0=0, **knots):
        k = [10.0] * 16
        for i, v in knots.items():
            k[int(i[1:])] = v
        return L.YuvDegradeNoise(3, t0, (C.c_float * 16)(*k))

    ok = noise()
    fb8 = f8.frame_bytes(40, 72)
    refused = [
        (None, f8, ok, gauss, dst, 1, 40, 72), (src, None, ok, gauss, dst, 1, 40, 72), (src, f8, None, gauss, dst, 1, 40, 72),      # null pointers
        (src, f8, ok, None, dst, 1, 40, 72), (src, f8, ok, gauss, None, 1, 40, 72),
        (src, yuv_fmt(12, 0, 0, 0), ok, gauss, dst, 1, 40, 72), (src, yuv_fmt(8, 3, 0, 0), ok, gauss, dst, 1, 40, 72),              # bits, chroma code
        (src, yuv_fmt(8, 0, 2, 0), ok, gauss, dst, 1, 40, 72), (src, yuv_fmt(8, 0, 0, 2), ok, gauss, dst, 1, 40, 72),               # matrix, range
        (src + 1, f10, ok, gauss, dst, 1, 40, 72), (src, f10, ok, gauss, dst + 1, 1, 40, 72),                                       # 10 bit: an odd address
        (src, f8, ok, gauss + 2, dst, 1, 40, 72),                                                                                   # gauss not 4-byte aligned
        (src, f8, noise(t0=-1), gauss, dst, 1, 40, 72),                                                                             # t0
        (src, f8, noise(k0=-1.0), gauss, dst, 1, 40, 72), (src, f8, noise(k15=float("nan")), gauss, dst, 1, 40, 72),                # a knot
        (src, f8, noise(k7=float("inf")), gauss, dst, 1, 40, 72),
        (src, f8, ok, gauss, src, 1, 40, 72), (src, f8, ok, gauss, src + fb8, 2, 40, 72), (src + 2 * fb8 - 1, f8, ok, gauss, src, 2, 40, 72),      # overlap
        (src, f8, ok, gauss, dst, 0, 40, 72), (src, f8, ok, gauss, dst, 65536, 40, 72),                                             # T
        (src, f8, ok, gauss, dst, 1, 0, 72), (src, f8, ok, gauss, dst, 1, 40, 0),                                                   # H, W
        (src, f8, ok, gauss, src + (1 << 30), 1, 2 * 8 * 65535 + 1, 8),                                                                        # more rows of workgroups than a grid has
    ]
    for args in refused:
        n = args[2]
        assert lib.sn_yuv_degrade(args[0], args[1], None if n is None else C.byref(n), *args[3:], None) == -22, args
