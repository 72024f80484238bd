"""Float64 re-statement of the VQGAN encoder kernels of ``csrc/kernels/conv.hip`` that the decoder does not have
(``conv3x3(down=True)``, ``conv_in_rgb``, ``linear_argmax``), in the kernels' own layouts, beside ``vqgan_ref.py``
(which this module imports and leaves as it is). Plain torch, any device; used only by tests
(``test_vqgan_enc_ref_cpu.py`` pins these functions to ``torch.nn.functional``; ``test_vqgan_encoder_kernels_gpu.py``
judges the kernels against them element by element).

As in ``vqgan_ref``, every function upcasts what it is given, and the convolutions also return the magnitude
convolution ``A`` that scales the worst-case accumulation error.
"""
import math

import torch

import vqgan_ref as vr


def conv_down_ref(x, w, bias=None):
    """taming's Downsample: zero pad (0, 1, 0, 1) (right / bottom), then 3x3 / stride 2 / pad 0: output pixel (y, x)
    reads source (2y + ky, 2x + kx), zero where the index equals H or W.

    x (N, H, W, Cin) with even H, W; w (Cout, 9 * Cin) tap-major / channel-contiguous; bias (Cout) or None.
    Returns float64 (R, A), both (N, H / 2, W / 2, Cout)."""
    n, h, wd, cin = x.shape
    assert h % 2 == 0 and wd % 2 == 0
    ho, wo = h // 2, wd // 2

    def taps(xa, wa):
        xp = torch.nn.functional.pad(xa, (0, 0, 0, 1, 0, 1))  # one zero column on the right, one zero row below
        out = None
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            t = xp[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2, :] @ wa[:, tap * cin:(tap + 1) * cin].t()
            out = t if out is None else out + t
        return out

    xa, wa = x.double(), w.double()
    r, a = taps(xa, wa), taps(xa.abs(), wa.abs())
    if bias is not None:
        r = r + bias.double()
        a = a + bias.double().abs()
    return r, a


def rgb_rescale(images):
    """What ``conv_in_rgb`` convolves: bf16(fp32(2 x - 1)) of the fp32 images, as float64 (same shape)."""
    x = images.float()
    return (2.0 * x - 1.0).to(torch.bfloat16).double()


def conv_in_rgb_ref(images, w, bias):
    """images (N, 3, H, W) in [0, 1], w (Cout, 27) tap-major / channel-contiguous, bias (Cout):
    3x3 / stride 1 / zero pad 1 convolution of x' = bf16(fp32(2 x - 1)) plus bias.
    Returns float64 (R, A), both NHWC (N, H, W, Cout)."""
    xa = rgb_rescale(images).permute(0, 2, 3, 1).contiguous()
    return vr.conv3x3_ref(xa, w, bias)


def linear_argmax_ref(x, w, bias):
    """x (M, K), w (V, K), bias (V): float64 logits x w^T + bias and their magnitudes A = |x| |w|^T + |bias|,
    both (M, V)."""
    xd, wd, bd = x.double(), w.double(), bias.double()
    return xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()


# ---------------------------------------------------------------------------------------------------------------
# test cases shared by the GPU kernel test; inputs are already rounded to what the kernels read.
# conv3x3(down=True): (N, H, W, Cin, Cout), H and W are INPUT sizes. (1, 2, 256): every output pixel reads the bottom
# pad row; (1, 256, 2): every output pixel reads the right pad column.
DOWN_SHAPES = [(2, 16, 32, 128, 128), (1, 32, 16, 256, 256), (1, 2, 256, 128, 128), (1, 256, 2, 128, 128),
               (3, 32, 32, 128, 256)]
# conv_in_rgb: (N, H, W, Cout)
RGB_SHAPES = [(2, 8, 16, 128), (1, 1, 128, 128), (1, 128, 1, 128), (1, 16, 24, 256)]
# linear_argmax: (M, K, V)
ARGMAX_SHAPES = [(130, 64, 128), (256, 256, 384), (257, 256, 8192)]


def make_down_case(shape, has_bias):
    """Image n of the batch is (n + 1) * randn + 2 n, so a wrong image index is far out of bound."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(sum(v * 131 ** i for i, v in enumerate(shape)) % (2 ** 31))
    nn = torch.arange(n, dtype=torch.float32)[:, None, None, None]
    x = ((nn + 1) * torch.randn(n, h, w, cin, generator=g) + 2 * nn).to(torch.bfloat16)
    wk = ((torch.rand(cout, 9 * cin, generator=g) * 2 - 1) / math.sqrt(9 * cin)).to(torch.bfloat16)
    bias = (torch.rand(cout, generator=g) - 0.5) if has_bias else None
    return x, wk, bias


def make_rgb_case(shape):
    """Images in [0, 1] that contain exact 0.0 and 1.0 (about a tenth of the pixels each); image n is scaled towards
    a level of its own, n / (N + 1), so a wrong image index shows."""
    n, h, w, cout = shape
    g = torch.Generator().manual_seed(sum(v * 137 ** i for i, v in enumerate(shape)) % (2 ** 31))
    u = torch.rand(n, 3, h, w, generator=g)
    lvl = torch.arange(n, dtype=torch.float32)[:, None, None, None] / (n + 1)
    img = (lvl + (1 - lvl) * u).clamp(0, 1)
    sel = torch.rand(n, 3, h, w, generator=g)
    img = torch.where(sel < 0.1, torch.zeros(()), img)
    img = torch.where(sel > 0.9, torch.ones(()), img)
    wk = ((torch.rand(cout, 27, generator=g) * 2 - 1) / math.sqrt(27)).to(torch.bfloat16)
    bias = torch.rand(cout, generator=g) - 0.5
    return img.contiguous(), wk, bias


def make_argmax_case(shape):
    m, k, v = shape
    g = torch.Generator().manual_seed(sum(d * 139 ** i for i, d in enumerate(shape)) % (2 ** 31))
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    w = (torch.randn(v, k, generator=g) / math.sqrt(k)).to(torch.bfloat16)
    bias = torch.randn(v, generator=g) * 0.1
    return x, w, bias


# ---------------------------------------------------------------------------------------------------------------
# the small VQGAN of test_vqgan_gpu.py, shared by the CPU emulation test and the GPU encoder test (same seed, same
# weights and pictures on both)
DDCONFIG = dict(ch=128, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=(16,), resolution=64,
                z_channels=256)
N_EMBED = 512


def small_vae(is_gumbel):
    from dalle_amd.models.vqgan import VQGanVAE

    torch.manual_seed(0)
    return VQGanVAE(n_embed=N_EMBED, embed_dim=256, ddconfig=DDCONFIG, is_gumbel=is_gumbel).eval()


def small_images(n=3, side=64):
    return torch.rand(n, 3, side, side, generator=torch.Generator().manual_seed(1))


@torch.no_grad()
def latent(vae, images):
    """The pre-quantisation latent ``quant_conv(encoder(2 x - 1))``, NCHW."""
    return vae.quant_conv(vae.encoder(2 * images - 1))


@torch.no_grad()
def latent_bf16_emulated(vae, images):
    """The same latent from a copy of the model whose convolutions (3x3 and 1x1) read bf16-rounded inputs and
    bf16-rounded weights, everything else fp32: the roundings any bf16-operand encoder makes at its matrix products,
    without a single line of the HIP path."""
    import copy

    m = copy.deepcopy(vae)
    convs = [c for c in list(m.encoder.modules()) + [m.quant_conv] if isinstance(c, torch.nn.Conv2d)]
    for c in convs:
        c.weight.copy_(vr.bf16_round(c.weight))
        c.register_forward_pre_hook(lambda mod, args: (vr.bf16_round(args[0]),))
    return latent(m, images)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()
