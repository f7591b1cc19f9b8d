"""Checkpoint tensors prepared once per device.  ``PlanBase`` walks the checkpoint (which convs, CABs and GSTS units a variant has, under which names);
``Plan`` packs them into the bf16 kernels' layouts (prep.py), ``engine32.Plan32`` keeps the fp32 values."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import lib as L
from . import prep
from .spec import UNIT_NAMES, Variant, shift_table


def host_f32_copy(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """fp32 CPU copies of a state dict with ONE device-to-host transfer: the ~2000 tensors of a checkpoint are flattened into one
    buffer on their device first (per-key .cpu() calls cost 5755 copyBuffer launches / 27 ms per plan build in the round-2 profile)."""
    keys = list(sd.keys())
    if not keys:
        return {}
    dev_keys = [k for k in keys if sd[k].device.type != "cpu"]
    out = {k: sd[k].detach().float() for k in keys if sd[k].device.type == "cpu"}
    if dev_keys:
        flat = torch.cat([sd[k].detach().reshape(-1).float() for k in dev_keys]).cpu()
        o = 0
        for k in dev_keys:
            n = sd[k].numel()
            out[k] = flat[o:o + n].reshape(sd[k].shape)
            o += n
    return {k: out[k] for k in keys}


class PlanBase:
    """The checkpoint walk and the entries both plans store alike.  A plan implements add_conv, add_cab and add_naf."""

    def __init__(self, V: Variant, sd: Dict[str, torch.Tensor], device: torch.device) -> None:
        self.V = V
        self.device = device
        self.sd = host_f32_copy(sd)
        self.convs: Dict[str, Dict[str, object]] = {}
        self.cas: Dict[str, Dict[str, object]] = {}
        self.units: Dict[str, Dict[str, object]] = {}
        self.offs = prep.shift_offsets_i8(shift_table(V.c1)).to(device)
        self._build()

    def _dev(self, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        return None if t is None else t.contiguous().to(self.device)

    def add_ca(self, name: str, key: str) -> None:
        wa = self.sd[key + "conv_du.0.weight"]
        wb = self.sd[key + "conv_du.2.weight"]
        cr, c = wa.shape[0], wa.shape[1]
        self.cas[name] = {"wa": self._dev(wa.reshape(cr, c)), "wb": self._dev(wb.reshape(c, cr)), "c": c, "cr": cr}

    def scalar(self, key: str) -> float:
        return float(self.sd[key].reshape(-1)[0])

    def add_shift_block(self, pre: str, c: int) -> None:
        for k in range(self.V.units):
            self.add_naf(f"{pre}{UNIT_NAMES[k]}.0.", c, True)
            self.add_naf(f"{pre}{UNIT_NAMES[k]}.1.", c, False)

    def add_down(self, pre: str, cin: int) -> None:
        self.add_conv(pre + "down", pre + ("down.0." if self.V.denoise else "down."), [cin])

    def add_unet(self, pre: str) -> None:
        V = self.V
        c = [V.c0, V.c0 + V.unet_step, V.c0 + 2 * V.unet_step]
        for lvl, n in ((1, 1), (2, 3), (3, 3)):
            for i in range(n):
                self.add_cab(f"{pre}encoder_level{lvl}.{i}.", c[lvl - 1])
                self.add_cab(f"{pre}decoder_level{lvl}.{i}.", c[lvl - 1])
        self.add_down(pre + "down12.", c[0])
        self.add_down(pre + "down23.", c[1])
        self.add_cab(pre + "skip_attn1.", c[0])
        self.add_cab(pre + "skip_attn2.", c[1])
        self.add_conv(pre + "up21", pre + "up21.up.1.", [c[1]])
        self.add_conv(pre + "up32", pre + "up32.up.1.", [c[2]])

    def _build(self) -> None:
        V = self.V
        c0, c1 = V.c0, V.c1
        self.add_conv("feat_extract.0", "feat_extract.0.", [V.in_ch])
        self.add_cab("feat_extract.1.", c0)
        self.add_conv("conv_trans", "conv_trans.", [c0])
        self.add_conv("conv_last", "conv_last.", [c0])
        self.add_conv("rconcat", "rconcat.", [c0, c0, c0])
        for i in range(1, V.n_orb + 1):
            self.add_unet(f"orb{i}.")
            self.add_unet(f"rorb{i}.")
        p = "stage1."
        self.add_cab(p + "concat.", c0)
        self.add_conv(p + "down01", p + "down01.0.", [c0])
        self.add_down(p + "down12.", c1)
        if V.topo == "small":
            blocks = ["encoder_level1", "encoder_level1_1", "encoder_level1_2", "encoder_level2", "encoder_level2_1",
                      "encoder_level2_2", "decoder_level2", "decoder_level2_1", "decoder_level2_2",
                      "decoder_level1", "decoder_level1_1", "decoder_level1_2"]
        else:
            self.add_down(p + "down23.", c1)
            if V.shift_cab:
                self.add_cab(p + "encoder_level0.", c0)
                self.add_cab(p + "encoder_level0_1.", c0)
            for n in ("encoder_level1", "encoder_level1_1", "encoder_level2", "encoder_level2_1",
                      "encoder_level3", "encoder_level3_1"):
                self.add_cab(f"{p}{n}.", c1)
            self.add_cab(p + "skip_attn2.", c1)
            self.add_conv(p + "up32", p + "up32.up.1.", [c1])
            blocks = ["decoder_level3", "decoder_level3_1", "decoder_level2", "decoder_level2_1",
                      "decoder_level1", "decoder_level1_1", "decoder_level1_2"]
        for b in blocks:
            self.add_shift_block(f"{p}{b}.", c1)
        self.add_cab(p + "skip_attn1.", c1)
        self.add_conv(p + "up21", p + "up21.up.1.", [c1])
        self.add_conv(p + "upsample0", p + "upsample0.upsample_conv.", [c1], shuffle=True)
        self.add_cab(p + "skip_conv.", c0)
        self.add_cab(p + "out_conv.", c0)
        self.add_conv(p + "conv_hr0", p + "conv_hr0.", [c0, c0] if V.hr_cat else [c0])


class Plan(PlanBase):
    """Device-resident prepared weights of one checkpoint in the bf16 kernels' layouts."""

    # "<block prefix><operand>" of the first fused phase-1 operand (w3, wgrp, wfrag2) whose fp16 packing is not finite, or None.  The gate's rescaling
    # symmetry lets a checkpoint hold small body.0 rows against a large second 1x1 (times 1 / P1_G1_SCALE in wfrag2); Engine starts such a module on the
    # two-kernel chain, whose second 1x1 is bf16.
    p1r_not_finite: Optional[str] = None

    def __init__(self, V: Variant, sd: Dict[str, torch.Tensor], device: torch.device) -> None:
        super().__init__(V, sd, device)
        # sn_gsts_shiftconv_mfma reads 16 bytes of a channel-planar LDS row at a displaced column: 8-byte aligned only if every displacement is a multiple
        # of 4 pixels (gshift_deblur1.py:411-439: they are 0, +-4, +-8) and within the 34 x 34 window; anything else stays on the VALU kernel
        self.k0_mfma_ok = all(dx % 4 == 0 and abs(dy) <= 8 and abs(dx) <= 8 for dy, dx in shift_table(V.c1))

    def add_conv(self, name: str, key: str, cins: Sequence[int], shuffle: bool = False) -> None:
        w = self.sd[key + "weight"]
        b = self.sd.get(key + "bias")
        cs_in = prep.ceil8(max(cins))
        p = prep.pack_conv(w, b, cins, cs_in, shuffle)
        p["wfrag"] = self._dev(p["wfrag"])
        p["bias"] = self._dev(p["bias"])
        self.convs[name] = p

    def add_cab(self, pre: str, c: int) -> None:
        self.add_conv(pre + "body.0", pre + "body.0.", [c])
        self.add_conv(pre + "body.2", pre + "body.2.", [c])
        self.add_ca(pre + "CA", pre + "CA.")
        # fp32 [cin][9][cpad] copy of the second conv for the closed-form pooled mean of res (sn_cab_ca); bf16-rounded like the MFMA operand
        cpad = 16 * int(self.convs[pre + "body.2"]["mt"])
        w2 = torch.zeros((c, 9, cpad), dtype=torch.float32)
        w2[:, :, :c] = self.sd[pre + "body.2.weight"].to(torch.bfloat16).float().reshape(c, c, 9).permute(1, 2, 0)
        self.cas[pre + "CA"]["w2"] = self._dev(w2)

    def add_naf(self, pre: str, c: int, with_shift: bool) -> None:
        V, sd = self.V, self.sd
        u: Dict[str, object] = {}
        i = 0
        if with_shift:
            w1 = sd[pre + "conv1.weight"].reshape(c // 2, 9)
            u["w1"] = self._dev((w1.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF).contiguous())   # bf16 in the low half
        g = prep.pack_ln_gemm(sd[f"{pre}body.{i}.weight"], sd[pre + "norm.weight"], sd[pre + "norm.bias"], c); i += 1
        u["w_ln"], u["b_ln"] = self._dev(g["wfrag"]), self._dev(g["bias"])
        w3 = prep.pack_dw3_gate(sd[f"{pre}body.{i}.conv_2.weight"], c); i += 1
        if not bool(torch.isfinite(w3.to(torch.float16)).all()):
            raise ValueError(f"shiftnet_amd: {pre}body.1.conv_2.weight is not finite in fp16 (w_dw3_h2, the packed stencil of sn_ln_gemm_gate): neither phase-1 "
                             "path can run this checkpoint in half precision -- run the module in float32 (net.float(): the fp32 engine has no fp16 operands)")
        u["w_dw3_h2"] = self._dev(prep.pk_f16_words(w3))        # K12: packed-fp16 stencil, [9][C] words = positions (2k, 2k+1)
        i += 1
        if V.denoise:
            self.add_ca(f"{pre}ca1", f"{pre}body.{i}."); i += 1
        if V.grouped_rep:
            u["w_grp"] = self._dev(prep.pack_grouped_frag(sd[f"{pre}body.{i}.conv_1.weight"], sd[f"{pre}body.{i}.conv_2.weight"]))
        else:
            w5 = prep.pack_dw5(sd[f"{pre}body.{i}.conv_1.weight"], sd[f"{pre}body.{i}.conv_2.weight"])
            u["w_toep5"] = self._dev(prep.pack_toeplitz(w5, 5))           # K3m: 5x5 on the matrix cores
        i += 1
        u["w_gate"] = self._dev(prep.pack_gate_gemm(sd[f"{pre}body.{i}.weight"], c))
        # fused phase 1 (sn_gsts_cab2_phase1 / sn_cab1_phase1, csrc/sn_phase1r.hip); the denoisers run it twice (inner CALayer2: sn_phase1_opts)
        pk = prep.pack_phase1r(
            sd[f"{pre}body.0.weight"], sd[pre + "norm.weight"], sd[pre + "norm.bias"], sd[f"{pre}body.1.conv_2.weight"],
            sd[f"{pre}body.{i - 1}.conv_1.weight"], sd[f"{pre}body.{i - 1}.conv_2.weight"], sd[f"{pre}body.{i}.weight"], c)
        if self.p1r_not_finite is None:
            self.p1r_not_finite = next((pre + k for k in ("w3", "wgrp", "wfrag2") if not bool(torch.isfinite(pk[k].view(torch.float16)).all())), None)
        d = {k: self._dev(v) for k, v in pk.items()}
        d["desc"] = L.Phase1Weights(d["wfrag1"].data_ptr(), d["w3"].data_ptr(), d["wgrp"].data_ptr(), d["wfrag2"].data_ptr())   # the tensors stay referenced in d
        u["p1r"] = d
        i += 1
        i += 1
        self.add_ca(f"{pre}ca2", f"{pre}body.{i}."); i += 1
        o = prep.pack_out_gemm(sd[f"{pre}body.{i}.weight"], sd[pre + "beta"], sd.get(f"{pre}body.{i}.bias"), c)
        u["w_out"], u["b_out"] = self._dev(o["wfrag"]), self._dev(o["bias"])
        self.units[pre] = u
