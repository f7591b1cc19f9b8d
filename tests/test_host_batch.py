"""Batched multi-clip forward (GShiftNet.forward_clips), host side: argument validation, the CLI flag and the ABI 19 descriptors.

No GPU: validation happens before the module looks for its device, so a CPU module reports a bad argument first and the missing device
("no CPU fallback") only for a well-formed call.  tests/test_gpu_batch.py checks the results on the MI355X.
"""
import pytest
import torch

from shiftnet_amd import cli
from shiftnet_amd import lib as L
from shiftnet_amd.arch import CLASSES

VARIANTS = ["gshift_deblur1", "gshift_deblur2", "gshift_denoise1", "gshift_denoise2"]


def _net(name, dtype=torch.float32):
    return CLASSES[name]().to(dtype).eval()


def _call(net, name, x, nm="auto", fp32_out=False, **kw):
    denoise = "denoise" in name
    if nm == "auto":
        nm = torch.zeros(x.shape[:2] + (1,) + x.shape[3:], dtype=x.dtype) if denoise and x.dim() == 5 else None
    args = (x, nm) if denoise else (x,)
    return (net.forward_clips_fp32_out if fp32_out else net.forward_clips)(*args, **kw)


@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("fp32_out", [False, True])
def test_forward_clips_rejects_non_5d_input(name, fp32_out):
    net = _net(name)
    for shape in [(6, 3, 16, 16), (2, 2, 6, 3, 16, 16), (3, 16, 16)]:
        x = torch.zeros(shape)
        with pytest.raises(ValueError, match=r"\[B,T,C,H,W\]"):
            _call(net, name, x, nm=torch.zeros(1) if "denoise" in name else None, fp32_out=fp32_out)


@pytest.mark.parametrize("name", VARIANTS)
def test_forward_clips_rejects_dtype_mismatch(name):
    net = _net(name, torch.float32)
    with pytest.raises(RuntimeError, match="should be the same"):
        _call(net, name, torch.zeros(2, 5, 3, 16, 16, dtype=torch.bfloat16))
    net16 = _net(name, torch.float16)
    with pytest.raises(RuntimeError, match="should be the same"):
        _call(net16, name, torch.zeros(2, 5, 3, 16, 16))


@pytest.mark.parametrize("name", ["gshift_denoise1", "gshift_denoise2"])
@pytest.mark.parametrize("fp32_out", [False, True])
def test_forward_clips_denoise_needs_noise_map(name, fp32_out):
    net = _net(name)
    with pytest.raises(TypeError, match="noise_map is required"):
        _call(net, name, torch.zeros(2, 5, 3, 16, 16), nm=None, fp32_out=fp32_out)


@pytest.mark.parametrize("name", ["gshift_deblur1", "gshift_deblur2"])
def test_forward_clips_deblur_takes_no_noise_map(name):
    net = _net(name)
    x = torch.zeros(2, 5, 3, 16, 16)
    with pytest.raises(TypeError):
        net.forward_clips(x, torch.zeros(2, 5, 1, 16, 16))
    with pytest.raises(TypeError):                                    # (its second positional argument is the shortcut, as in forward_fp32_out)
        net.forward_clips_fp32_out(x, noise_map=torch.zeros(2, 5, 1, 16, 16))


@pytest.mark.parametrize("name", VARIANTS)
def test_forward_clips_shortcut_shape_is_checked(name):
    net = _net(name)
    x = torch.zeros(2, 5, 3, 16, 16)
    with pytest.raises(ValueError, match="shortcut"):
        _call(net, name, x, fp32_out=True, shortcut=torch.zeros(5, 3, 16, 16))
    with pytest.raises(ValueError, match="shortcut"):
        _call(net, name, x, fp32_out=True, shortcut=torch.zeros(1, 5, 3, 16, 16))


@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("fp32_out", [False, True])
def test_forward_clips_cpu_module_has_no_fallback(name, fp32_out):
    net = _net(name)
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:
        _call(net, name, torch.zeros(2, 5, 3, 16, 16), fp32_out=fp32_out)
    with pytest.raises(RuntimeError, match="no CPU fallback") as f:                     # the same error as forward's
        net(torch.zeros(2, 5, 3, 16, 16), torch.zeros(2, 5, 1, 16, 16)) if "denoise" in name else net(torch.zeros(2, 5, 3, 16, 16))
    assert str(e.value) == str(f.value)


def test_forward_clips_refuses_a_temporal_split():
    net = _net("gshift_deblur2")
    net.set_temporal_split(0, 2)
    with pytest.raises(ValueError, match="temporal split"):
        net.forward_clips(torch.zeros(2, 5, 3, 16, 16))
    net.set_temporal_split(0, 1)                                      # back to one rank: the call reaches the device check again
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.forward_clips(torch.zeros(2, 5, 3, 16, 16))


@pytest.mark.parametrize("name", VARIANTS)
def test_batch_quadrants_flag_only_on_denoise_clis(name):
    ap = cli.make_parser(name)
    if "denoise" in name:
        assert ap.parse_args([]).batch_quadrants is False            # off by default
        assert ap.parse_args(["--batch_quadrants"]).batch_quadrants is True
    else:
        with pytest.raises(SystemExit):
            ap.parse_args(["--batch_quadrants"])


def test_abi20_descriptors_carry_the_clip_fields_zeroed():
    """The clip fields arrived with ABI 19; ABI 20 (sn_conv2d_route) kept both descriptors' layouts."""
    assert L.ABI_VERSION == 20
    s = L.UnitSrc()
    assert s.clip == 0
    s = L.UnitSrc(None, 12, 8, 8, 64, 1, 0, None, 0, 0, 6)           # positional: clip comes last
    assert s.clip == 6 and s.nt == 0
    for cls in (L.ConvDesc, L.Conv32Desc):
        d = cls()
        assert (d.clip_n, d.clip_T, d.clip_lo) == (0, 0, 0)
        names = [f[0] for f in cls._fields_]
        assert names[-3:] == ["clip_n", "clip_T", "clip_lo"]
    assert [f[0] for f in L.UnitSrc._fields_][-1] == "clip"
