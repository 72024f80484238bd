"""Float64 re-statement of the VQGAN decoder kernels of ``csrc/kernels/conv.hip`` (``conv3x3``, ``gn_stats``,
``gn_apply``, ``conv_out``, ``softmax_rows``) in the kernels' own layouts: NHWC activations, 3x3 weights as
``(Cout, 9 * Cin)`` tap-major / channel-contiguous, GroupNorm ``mean`` / ``rstd`` as ``(N, 32)``. Plain torch, any
device. Used only by tests (``test_vqgan_ref_cpu.py`` pins these functions to ``torch.nn.functional``;
``test_vqgan_kernels_gpu.py`` judges the kernels against them element by element).

Every function upcasts what it is given: hand it the bf16-rounded activations / weights and the fp32 statistics the
kernel reads, and input rounding is never charged to the kernel. The convolutions also return the magnitude
convolution ``A = conv(|x'|, |w|) + |bias| + |res|`` that scales the worst-case accumulation error.

``act_dtype=torch.float32`` evaluates SiLU(GN(x)) of the same emulation in fp32 (everything after its bf16 rounding
stays float64); the difference from the float64 result measures what a correct fp32 implementation pays for the
flips of that rounding, see ``measure_gn_constant``.
"""
import math

import torch

GROUPS = 32


def bf16_round(t):
    """Round to bf16 (nearest even), keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def _per_channel(stat, c, dtype):
    """(N, 32) per-group statistic -> (N, 1, 1, C)."""
    return stat.to(dtype).repeat_interleave(c // GROUPS, dim=1)[:, None, None, :]


def _silu(v):
    return v * torch.sigmoid(v)


def gn_stats_ref(x, eps):
    """x (N, H, W, C) -> float64 (mean, rstd, E|x|, E[x^2]), each (N, 32); biased variance, as GroupNorm."""
    n, h, w, c = x.shape
    xd = x.double().reshape(n, h * w, GROUPS, c // GROUPS)
    mean = xd.mean(dim=(1, 3))
    var = (xd - mean[:, None, :, None]).square().mean(dim=(1, 3))
    rstd = (var + eps).rsqrt()
    return mean, rstd, xd.abs().mean(dim=(1, 3)), xd.square().mean(dim=(1, 3))


def gn_apply_ref(x, mean, rstd, gamma, beta, silu):
    """(x - mean) * rstd * gamma + beta, optionally through SiLU; float64 (N, H, W, C)."""
    c = x.shape[-1]
    v = (x.double() - _per_channel(mean, c, torch.float64)) * _per_channel(rstd, c, torch.float64) * gamma.double()
    v = v + beta.double()
    return _silu(v) if silu else v


def _gn_silu(x, gn, dtype):
    """SiLU(GroupNorm(x)) as per-channel scale / shift of the image (the form the convolutions apply)."""
    mean, rstd, gamma, beta = gn
    c = x.shape[-1]
    sc = _per_channel(rstd, c, dtype) * gamma.to(dtype)
    sh = beta.to(dtype) - _per_channel(mean, c, dtype) * sc
    return _silu(x * sc + sh)


def _conv_taps(xp, w, h, wd):
    """sum over the 9 taps of xp[:, y + ky, x + kx, :] @ w[:, tap]^T; xp is zero-padded by one pixel."""
    cin = xp.shape[-1]
    out = None
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        t = xp[:, ky:ky + h, kx:kx + wd, :] @ w[:, tap * cin:(tap + 1) * cin].t()
        out = t if out is None else out + t
    return out


def _pad1(x):
    return torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))


def conv3x3_ref(x, w, bias=None, res=None, gn=None, ups=False, round_act=False, act_dtype=torch.float64):
    """3x3 / stride 1 / zero pad 1 convolution of x' = upsample2x(SiLU(GN(x))) (each stage optional).

    x (N, Hs, Ws, Cin), w (Cout, 9 * Cin), bias (Cout) or None, res (N, H, W, Cout) or None,
    gn = (mean, rstd, gamma, beta) or None. ``round_act`` rounds SiLU(GN(x)) to bf16 before the convolution, as the
    kernel's gather (and the ``gn_apply`` pre-pass) does. Returns float64 (R, A), both (N, H, W, Cout)."""
    dtype = torch.float64
    xa = x.to(dtype)
    if gn is not None:
        xa = _gn_silu(x.to(act_dtype), gn, act_dtype)
        if round_act:
            xa = bf16_round(xa)
        xa = xa.to(dtype)
    if ups:
        xa = xa.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    h, wd = xa.shape[1], xa.shape[2]
    wa = w.to(dtype)
    r = _conv_taps(_pad1(xa), wa, h, wd)
    a = _conv_taps(_pad1(xa.abs()), wa.abs(), h, wd)
    if bias is not None:
        r = r + bias.to(dtype)
        a = a + bias.to(dtype).abs()
    if res is not None:
        r = r + res.to(dtype)
        a = a + res.to(dtype).abs()
    return r, a


def conv_out_ref(x, w, bias, mean, rstd, gamma, beta):
    """Final GroupNorm + SiLU + 3x3 conv to 3 channels. x (N, H, W, C), w (3, 9 * C), bias (3).
    Returns float64 (pre-clamp value, image (clamp(-1, 1) + 1) / 2, A), each NCHW (N, 3, H, W)."""
    pre, a = conv3x3_ref(x, w, bias, None, gn=(mean, rstd, gamma, beta))
    pre, a = pre.permute(0, 3, 1, 2).contiguous(), a.permute(0, 3, 1, 2).contiguous()
    return pre, (pre.clamp(-1.0, 1.0) + 1.0) * 0.5, a


def softmax_rows_ref(s, scale):
    """softmax over the last axis of s * scale; the product is formed in float64 from the fp32 scores and the
    scale as the kernel receives it (rounded to fp32)."""
    sc = torch.tensor(float(scale), dtype=torch.float32).double().item()
    return torch.softmax(s.double() * sc, dim=-1)


# ---------------------------------------------------------------------------------------------------------------
# conv3x3 test cases, shared by the CPU measurement of the GroupNorm constant and the GPU kernel test.
# (N, H, W, Cin, Cout, ups): H, W are OUTPUT sizes.
SHAPES_CROSSED = [(2, 8, 16, 64, 128, False), (3, 16, 16, 192, 384, False), (2, 16, 16, 128, 128, True),
                  (1, 8, 32, 64, 256, True)]
SHAPES_SINGLE = [(1, 1, 128, 64, 128, False), (1, 128, 1, 64, 128, False), (1, 8, 16, 1024, 128, False),
                 (2, 16, 8, 128, 256, False)]


def conv_cases():
    """(N, H, W, Cin, Cout, ups, gn, bias, res): the crossed shapes with every GroupNorm / bias / residual setting,
    the others with GroupNorm off and on (bias and residual given)."""
    out = []
    for shp in SHAPES_CROSSED:
        for gn in (False, True):
            for bias in (False, True):
                for res in (False, True):
                    out.append(shp + (gn, bias, res))
    for shp in SHAPES_SINGLE:
        for gn in (False, True):
            out.append(shp + (gn, True, True))
    return out


GN_CASES = [c for c in conv_cases() if c[6]]


def make_conv_case(case, eps=1e-6):
    """Deterministic CPU inputs of one case, already rounded to what the kernel reads: x, w, res bf16; bias, gamma,
    beta and the GroupNorm statistics fp32 (the float64 reference statistics of the bf16 x, cast to fp32).
    Image n of the batch is (n + 1) * randn + 2 n, so a statistics table indexed with the wrong image is far off."""
    n, h, w, cin, cout, ups, gn, has_bias, has_res = case
    seed = 0
    for v in (n, h, w, cin, cout, int(ups)):
        seed = (seed * 131 + v) % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    hs, ws = (h // 2, w // 2) if ups else (h, w)
    x = torch.randn(n, hs, ws, cin, generator=g)
    nn = torch.arange(n, dtype=torch.float32)[:, None, None, None]
    x = ((nn + 1) * x + 2 * nn).to(torch.bfloat16)
    bound = 1.0 / math.sqrt(9 * cin)
    wk = ((torch.rand(cout, 9 * cin, generator=g) * 2 - 1) * bound).to(torch.bfloat16)
    bias = (torch.rand(cout, generator=g) - 0.5) if has_bias else None
    res = torch.randn(n, h, w, cout, generator=g).to(torch.bfloat16) if has_res else None
    gamma = torch.rand(cin, generator=g) + 0.5
    beta = torch.rand(cin, generator=g) * 0.6 - 0.3
    stats = None
    if gn:
        mean, rstd, _, _ = gn_stats_ref(x, eps)
        stats = (mean.float(), rstd.float(), gamma, beta)
    return dict(x=x, w=wk, bias=bias, res=res, gn=stats, ups=ups)


def measure_gn_constant(cases=None):
    """max over the GroupNorm cases and elements of |R32 - R| / A between the round_act emulation with SiLU(GN(x))
    evaluated in fp32 and in float64: what the flips of the activation's bf16 rounding cost a correct fp32 kernel."""
    worst = 0.0
    for case in (cases or GN_CASES):
        d = make_conv_case(case)
        r64, a = conv3x3_ref(d["x"], d["w"], d["bias"], d["res"], gn=d["gn"], ups=d["ups"], round_act=True)
        r32, _ = conv3x3_ref(d["x"], d["w"], d["bias"], d["res"], gn=d["gn"], ups=d["ups"], round_act=True,
                             act_dtype=torch.float32)
        worst = max(worst, ((r32 - r64).abs() / a).max().item())
    return worst
