"""VQGAN decoder and encoder on the hand-written HIP kernels (``csrc/kernels/conv.hip``).

Runs the taming ``Decoder`` / ``Encoder`` of :mod:`dalle_amd.models.vqgan` with NHWC bf16 activations:

* every 3x3 convolution is the implicit-GEMM MFMA kernel (``conv3x3``); a ResNet block is
  ``gn_stats -> conv3x3(GN+SiLU fused into its input gather) -> gn_stats -> conv3x3(GN+SiLU in,
  residual out)``, and the Upsample's 2x nearest interpolation is folded into its conv's gather;
* the 1x1 convolutions (``post_quant_conv``, the ``nin_shortcut`` of channel-changing blocks, the
  attention block's q/k/v/proj) are plain GEMMs over the NHWC pixels (hipBLASLt);
* the 32x32 attention block: ``gn_apply`` -> one qkv GEMM -> scores (fp32) -> ``softmax_rows`` ->
  P V -> proj + residual;
* ``conv_out``: final GroupNorm + SiLU + 3x3 conv to RGB + clamp / rescale, written as NCHW fp32;
* encoder (:class:`HipEncoder`): ``conv_in_rgb`` (the 2x - 1 rescale and the 3 -> ch conv, NCHW fp32 in), the same
  ResNet / attention blocks, ``conv3x3(down=True)`` for taming's Downsample (zero pad right / bottom, stride 2),
  ``quant_conv`` as a GEMM and ``linear_argmax`` for the code selection (Gumbel ``proj`` logits, or nearest
  codebook vector as ``argmax (z . e - |e|^2 / 2)``) without the (pixels, codes) matrix.

Weights are converted once (bf16, conv kernels as [Cout, 3*3*Cin] tap-major / channel-contiguous) and
cached on the module; the fp32 torch ``Decoder`` stays the numerics reference
(``tests/test_vqgan_gpu.py``).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import os

import torch
import torch.nn.functional as F

from .vqgan import AttnBlock, Decoder, Encoder, ResnetBlock, Upsample


def _conv_w(conv: torch.nn.Conv2d) -> torch.Tensor:
    w = conv.weight.detach()
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(torch.bfloat16).contiguous()


def _lin_w(conv: torch.nn.Conv2d) -> torch.Tensor:
    return conv.weight.detach().reshape(conv.weight.shape[0], -1).to(torch.bfloat16).contiguous()


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().float().contiguous()


# GroupNorm + SiLU as a separate bf16 pass ahead of the 3x3 conv for images of at least this many pixels (default 0:
# every GN conv; batch 64 decoder 45.0 -> 42.1 ms, the gain at the low-resolution / high-channel levels, neutral at
# 256 x 256: profiles/r6_vqgan_conv_out.txt). DALLE_AMD_VQGAN_GN_PREPASS=<pixels> keeps smaller images on the
# fused-gather form.
_GN_PREPASS_MIN_HW = int(os.environ.get("DALLE_AMD_VQGAN_GN_PREPASS", "0"))


class _HipBlocks:
    """The cached weights and the blocks the decoder and the encoder share."""

    def __init__(self):
        from ..ops.ext import load_extension

        self.C = load_extension(required=True)
        self._w: Dict[int, tuple] = {}

    # -- cached weights ------------------------------------------------------------------------
    def _gn(self, gn: torch.nn.GroupNorm):
        return _f32(gn.weight), _f32(gn.bias), float(gn.eps)

    def _cached(self, key, build):
        if key not in self._w:
            self._w[key] = build()
        return self._w[key]

    # -- blocks --------------------------------------------------------------------------------
    def conv3x3(self, x, conv, gn=None, res=None, ups=False):
        w, b = self._cached(id(conv), lambda: (_conv_w(conv), _f32(conv.bias)))
        if gn is None:
            return self.C.conv3x3(x, w, b, res, ups=ups)
        gamma, beta, eps = self._cached(id(gn), lambda: self._gn(gn))
        mean, rstd = self.C.gn_stats(x, eps)
        if x.shape[1] * x.shape[2] >= _GN_PREPASS_MIN_HW:
            # SiLU(GN(x)) once per element into bf16, then the plain conv: the fused form applies it in the gather,
            # i.e. 9 times per element (once per tap)
            return self.C.conv3x3(self.C.gn_apply(x, mean, rstd, gamma, beta, silu=True), w, b, res, ups=ups)
        return self.C.conv3x3(x, w, b, res, mean, rstd, gamma, beta, ups=ups)

    def linear(self, x, conv):
        """1x1 conv over NHWC pixels: (N, H, W, Cin) -> (N, H, W, Cout) (+ bias), one GEMM."""
        w, b = self._cached(id(conv), lambda: (_lin_w(conv), _f32(conv.bias)))
        n, h, wd, c = x.shape
        y = torch.mm(x.view(-1, c), w.t())
        if b is not None:
            y.add_(b.to(y.dtype))
        return y.view(n, h, wd, -1)

    def resblock(self, x, blk: ResnetBlock):
        h = self.conv3x3(x, blk.conv1, gn=blk.norm1)
        sc = x if blk.nin_shortcut is None else self.linear(x, blk.nin_shortcut)
        return self.conv3x3(h, blk.conv2, gn=blk.norm2, res=sc.contiguous())

    def attn(self, x, blk: AttnBlock):
        n, hh, ww, c = x.shape
        gamma, beta, eps = self._cached(id(blk.norm), lambda: self._gn(blk.norm))
        mean, rstd = self.C.gn_stats(x, eps)
        hn = self.C.gn_apply(x, mean, rstd, gamma, beta)
        wqkv, bqkv = self._cached(("qkv", id(blk)), lambda: (
            torch.cat([_lin_w(blk.q), _lin_w(blk.k), _lin_w(blk.v)]).contiguous(),
            torch.cat([_f32(blk.q.bias), _f32(blk.k.bias), _f32(blk.v.bias)]).contiguous()))
        qkv = torch.addmm(bqkv.to(torch.bfloat16), hn.view(-1, c), wqkv.t()).view(n, hh * ww, 3, c)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        s = torch.bmm(q, k.transpose(1, 2), out_dtype=torch.float32)
        p = self.C.softmax_rows(s, float(c) ** -0.5)
        o = torch.bmm(p, v)
        return x + self.linear(o.view(n, hh, ww, c), blk.proj_out)


class HipDecoder(_HipBlocks):
    """Executes ``post_quant_conv`` + ``decoder`` of a :class:`VQGanVAE` on MI355X."""

    def __init__(self, post_quant_conv: torch.nn.Conv2d, decoder: Decoder):
        super().__init__()
        self.dec = decoder
        self.pq = (_lin_w(post_quant_conv), _f32(post_quant_conv.bias))

    # -- whole decoder -------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, z_nhwc: torch.Tensor) -> torch.Tensor:
        """z (N, h, w, z_channels) bf16 -> images (N, 3, H, W) fp32 in [0, 1]."""
        d = self.dec
        n, hh, ww, c = z_nhwc.shape
        wpq, bpq = self.pq
        x = torch.addmm(bpq.to(torch.bfloat16), z_nhwc.reshape(-1, c), wpq.t()).view(n, hh, ww, -1)
        x = self.conv3x3(x.contiguous(), d.conv_in)
        x = self.resblock(x, d.mid.block_1)
        x = self.attn(x, d.mid.attn_1)
        x = self.resblock(x, d.mid.block_2)
        for i_level in reversed(range(d.num_resolutions)):
            up = d.up[i_level]
            for i_block in range(d.num_res_blocks + 1):
                x = self.resblock(x, up.block[i_block])
                if len(up.attn) > 0:
                    x = self.attn(x, up.attn[i_block])
            if i_level != 0:
                x = self.conv3x3(x, up.upsample.conv, ups=True)
        gamma, beta, eps = self._cached(id(d.norm_out), lambda: self._gn(d.norm_out))
        mean, rstd = self.C.gn_stats(x, eps)
        wout, bout = self._cached(id(d.conv_out), lambda: (_conv_w(d.conv_out), _f32(d.conv_out.bias)))
        return self.C.conv_out(x, wout, bout, mean, rstd, gamma, beta)


class HipEncoder(_HipBlocks):
    """Executes ``encoder`` + ``quant_conv`` + the code selection of a :class:`VQGanVAE` on MI355X."""

    def __init__(self, encoder: Encoder, quant_conv: torch.nn.Conv2d, quantize):
        super().__init__()
        self.enc = encoder
        self.quant_conv = quant_conv
        self.quantize = quantize

    def _bias(self, conv):
        b = conv.bias
        return torch.zeros(conv.out_channels, device=conv.weight.device) if b is None else _f32(b)

    @torch.no_grad()
    def latent(self, images: torch.Tensor) -> torch.Tensor:
        """images (N, 3, H, W) fp32 in [0, 1] -> the pre-quantisation latent (N, h, w, embed_dim) bf16 NHWC."""
        e = self.enc
        w, b = self._cached(id(e.conv_in), lambda: (_conv_w(e.conv_in), self._bias(e.conv_in)))
        x = self.C.conv_in_rgb(images.float().contiguous(), w, b)
        for i_level in range(e.num_resolutions):
            down = e.down[i_level]
            for i_block in range(e.num_res_blocks):
                x = self.resblock(x, down.block[i_block])
                if len(down.attn) > 0:
                    x = self.attn(x, down.attn[i_block])
            if i_level != e.num_resolutions - 1:
                conv = down.downsample.conv
                w, b = self._cached(id(conv), lambda: (_conv_w(conv), _f32(conv.bias)))
                x = self.C.conv3x3(x, w, b, down=True)
        x = self.resblock(x, e.mid.block_1)
        x = self.attn(x, e.mid.attn_1)
        x = self.resblock(x, e.mid.block_2)
        x = self.conv3x3(x, e.conv_out, gn=e.norm_out)
        return self.linear(x, self.quant_conv)

    def _selector(self):
        """(w (V, K) bf16, bias (V) fp32) of the argmax: the Gumbel quantiser's logit projection, or for a plain VQ
        the bf16 codebook with bias -|e|^2 / 2 taken in fp32 from the ROUNDED codebook, so operand and bias agree:
        argmin |z - e|^2 = argmax (z . e - |e|^2 / 2). Rebuilt when the parameters change."""
        q = self.quantize
        src = q.proj.weight if q.proj is not None else q.embed.weight
        key = (src.data_ptr(), src._version)
        if getattr(self, "_sel_key", None) != key:
            if q.proj is not None:
                self._sel = (_lin_w(q.proj), self._bias(q.proj))
            else:
                cb = q.embed.weight.detach().to(torch.bfloat16).contiguous()
                self._sel = (cb, (-0.5 * cb.float().square().sum(1)).contiguous())
            self._sel_key = key
        return self._sel

    @torch.no_grad()
    def codes_of(self, z_nhwc: torch.Tensor) -> torch.Tensor:
        """latent (N, h, w, K) bf16 -> code indices (N, h * w) int64."""
        n, hh, ww, k = z_nhwc.shape
        w, b = self._selector()
        return self.C.linear_argmax(z_nhwc.reshape(-1, k).contiguous(), w, b).view(n, hh * ww)

    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        return self.codes_of(self.latent(images))


def grid_supported(h: int, w: int) -> bool:
    """``conv3x3`` tiles 128 pixels of one image: every 3x3 conv's input pixel count must be a multiple of 128.
    The levels only upsample (x4 pixels each), so the latent grid decides it."""
    return h > 0 and w > 0 and (h * w) % 128 == 0


def supported(decoder: Decoder) -> bool:
    """The HIP path needs channel counts the kernels tile (multiples of 128 for the 3x3 convs, <= 128
    channels into the RGB conv) and 32-group GroupNorms. The code grid of a call is checked per call
    (:func:`grid_supported`)."""
    if any(m.num_groups != 32 for m in decoder.modules() if isinstance(m, torch.nn.GroupNorm)):
        return False
    convs: List[torch.nn.Conv2d] = [m for m in decoder.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]
    for m in convs:
        if m is decoder.conv_out:
            continue
        if m.in_channels % 64 or m.out_channels % 128:
            return False
    return decoder.conv_out.in_channels <= 128 and decoder.conv_out.in_channels % 32 == 0


def encoder_grid_supported(encoder: Encoder, h: int, w: int) -> bool:
    """Per call: the picture sides must halve ``levels - 1`` times and the latent grid must hold a multiple of 128
    pixels; every finer level has 4x the pixels of the next, so it tiles too (``conv_in_rgb`` and the stride-2
    ``conv3x3`` tile 128 output pixels of one image)."""
    f = 2 ** (encoder.num_resolutions - 1)
    return h > 0 and w > 0 and h % f == 0 and w % f == 0 and grid_supported(h // f, w // f)


def supported_encoder(encoder: Encoder, quant_conv: Optional[torch.nn.Conv2d] = None, quantize=None) -> bool:
    """The channel and group rules of :func:`supported` for the encoder's 3x3 convs (its ``conv_in`` reads RGB:
    ``in_channels == 3`` and an output width the kernel tiles), no ``double_z`` head, and -- when given -- a
    quantiser ``linear_argmax`` tiles (latent width % 64, code count % 128)."""
    if any(m.num_groups != 32 for m in encoder.modules() if isinstance(m, torch.nn.GroupNorm)):
        return False
    if encoder.conv_in.in_channels != 3 or encoder.conv_in.out_channels % 128:
        return False
    for m in encoder.modules():
        if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m is not encoder.conv_in:
            if m.in_channels % 64 or m.out_channels % 128 or m.in_channels > 1024:
                return False
    if quant_conv is not None:
        if encoder.conv_out.out_channels != quant_conv.in_channels:  # double_z: the head holds mean and log-variance
            return False
        if quantize is not None:
            v, k = quantize.embed.weight.shape
            if quantize.proj is not None:
                v, k = quantize.proj.out_channels, quantize.proj.in_channels
            if k != quant_conv.out_channels or k % 64 or v % 128:
                return False
    return True
