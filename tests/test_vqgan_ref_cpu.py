"""The float64 references of ``tests/vqgan_ref.py`` (what ``test_vqgan_kernels_gpu.py`` judges the VQGAN decoder
kernels against) agree with ``torch.nn.functional`` in float64 on the permuted tensors, and the per-element bounds of
the GPU test catch a reference that is wrong on the image border only or takes another image's GroupNorm table.
Also the predicates that decide which decoders and code grids take the HIP path."""
import pytest
import torch
import torch.nn.functional as F

import vqgan_ref as vr

TOL = 1e-12


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _w_oihw(w, cin):
    return w.double().reshape(w.shape[0], 3, 3, cin).permute(0, 3, 1, 2)


def _inputs(n, hs, ws, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    nn = torch.arange(n, dtype=torch.float64)[:, None, None, None]
    x = (nn + 1) * torch.randn(n, hs, ws, cin, generator=g, dtype=torch.float64) + 2 * nn
    w = torch.randn(cout, 9 * cin, generator=g, dtype=torch.float64) / (3 * cin ** 0.5)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    gamma = torch.rand(cin, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(cin, generator=g, dtype=torch.float64) * 0.6 - 0.3
    return x, w, bias, gamma, beta, g


@pytest.mark.parametrize("gn", [False, True])
@pytest.mark.parametrize("ups", [False, True])
@pytest.mark.parametrize("n,hs,ws,cin,cout", [(2, 5, 7, 32, 8), (3, 4, 4, 96, 16), (1, 1, 6, 64, 4)])
def test_conv3x3_ref_is_conv2d(n, hs, ws, cin, cout, ups, gn):
    eps = 1e-6
    x, w, bias, gamma, beta, g = _inputs(n, hs, ws, cin, cout, seed=cin + hs)
    h, wd = (2 * hs, 2 * ws) if ups else (hs, ws)
    res = torch.randn(n, h, wd, cout, generator=g, dtype=torch.float64)
    stats = None
    xin = _nchw(x)
    if gn:
        mean, rstd, _, _ = vr.gn_stats_ref(x, eps)
        stats = (mean, rstd, gamma, beta)
        xin = F.silu(F.group_norm(xin, 32, gamma, beta, eps))
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    want = F.conv2d(xin, _w_oihw(w, cin), bias, padding=1).permute(0, 2, 3, 1) + res
    want_a = F.conv2d(xin.abs(), _w_oihw(w, cin).abs(), bias.abs(), padding=1).permute(0, 2, 3, 1) + res.abs()
    got, got_a = vr.conv3x3_ref(x, w, bias, res, gn=stats, ups=ups)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert (got - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())
    assert (got_a - want_a).abs().max().item() <= TOL * max(1.0, want_a.abs().max().item())
    # without bias / residual
    got0, _ = vr.conv3x3_ref(x, w, None, None, gn=stats, ups=ups)
    assert (got0 - (want - res - bias)).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


def test_conv3x3_ref_round_act_rounds_the_activation():
    x, w, bias, gamma, beta, _ = _inputs(2, 4, 6, 64, 8, seed=3)
    mean, rstd, _, _ = vr.gn_stats_ref(x, 1e-6)
    act = vr.bf16_round(F.silu(F.group_norm(_nchw(x), 32, gamma, beta, 1e-6)))
    want = F.conv2d(act, _w_oihw(w, 64), bias, padding=1).permute(0, 2, 3, 1)
    got, _ = vr.conv3x3_ref(x, w, bias, None, gn=(mean, rstd, gamma, beta), round_act=True)
    # a flip of the bf16 rounding between the two float64 formulations would show as ~1e-3; none is expected
    assert (got - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("n,h,w,c", [(2, 5, 7, 32), (1, 4, 4, 96)])
def test_conv_out_ref_is_conv2d(n, h, w, c):
    x, wk, _, gamma, beta, g = _inputs(n, h, w, c, 3, seed=c)
    bias = torch.tensor([3.0, -3.0, 0.0], dtype=torch.float64)
    mean, rstd, _, _ = vr.gn_stats_ref(x, 1e-6)
    xin = F.silu(F.group_norm(_nchw(x), 32, gamma, beta, 1e-6))
    want = F.conv2d(xin, _w_oihw(wk, c), bias, padding=1)
    pre, img, a = vr.conv_out_ref(x, wk, bias, mean, rstd, gamma, beta)
    assert pre.shape == img.shape == a.shape == (n, 3, h, w)
    assert (pre - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())
    assert (img - (want.clamp(-1, 1) + 1) * 0.5).abs().max().item() <= TOL
    assert img.max().item() == 1.0 and img.min().item() == 0.0  # both clamp sides are reached
    want_a = F.conv2d(xin.abs(), _w_oihw(wk, c).abs(), bias.abs(), padding=1)
    assert (a - want_a).abs().max().item() <= TOL * max(1.0, want_a.abs().max().item())


@pytest.mark.parametrize("n,h,w,c", [(3, 1, 1, 32), (2, 5, 13, 96), (2, 4, 4, 2048)])
def test_gn_stats_ref_is_group_norm(n, h, w, c):
    eps = 1e-6
    g = torch.Generator().manual_seed(c)
    x = torch.randn(n, h, w, c, generator=g, dtype=torch.float64) * 2 + 5
    mean, rstd, eabs, esq = vr.gn_stats_ref(x, eps)
    xg = x.reshape(n, h * w, 32, c // 32)
    var, mu = torch.var_mean(xg, dim=(1, 3), unbiased=False)
    assert (mean - mu).abs().max().item() <= TOL * 10
    assert ((rstd - (var + eps).rsqrt()).abs() / rstd).max().item() <= 1e-9  # var by another formula: conditioning
    assert (eabs - xg.abs().mean(dim=(1, 3))).abs().max().item() <= TOL * 10
    assert (esq - (xg * xg).mean(dim=(1, 3))).abs().max().item() <= TOL * 100
    # and through the normalisation itself (a group of a single element normalises to beta)
    gamma = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(c, generator=g, dtype=torch.float64) - 0.5
    for silu in (False, True):
        want = F.group_norm(_nchw(x), 32, gamma, beta, eps)
        want = (F.silu(want) if silu else want).permute(0, 2, 3, 1)
        got = vr.gn_apply_ref(x, mean, rstd, gamma, beta, silu)
        assert (got - want).abs().max().item() <= TOL * 10


@pytest.mark.parametrize("scale", [1.0, 512 ** -0.5, 0.0])
@pytest.mark.parametrize("shape", [(1, 1), (5, 63), (5, 257), (2, 64, 64)])
def test_softmax_rows_ref_is_softmax(shape, scale):
    g = torch.Generator().manual_seed(7)
    s = torch.randn(*shape, generator=g) * 30
    sc32 = torch.tensor(scale, dtype=torch.float32).double()
    want = F.softmax(s.double() * sc32, dim=-1)
    got = vr.softmax_rows_ref(s, scale)
    assert got.dtype == torch.float64 and got.shape == s.shape
    assert (got - want).abs().max().item() <= TOL
    assert (got.sum(-1) - 1).abs().max().item() <= TOL


# ---------------------------------------------------------------------------------------------------------------
# the per-element conv bound has teeth: a reference that is wrong in one of the ways a gather kernel goes wrong,
# fed in place of the kernel's output, fails at every GroupNorm / upsample combination
def _crossed(gn, ups):
    return [c for c in vr.conv_cases() if c[6] == gn and c[5] == ups and c[7] and c[8]][0]


@pytest.mark.parametrize("gn", [False, True])
@pytest.mark.parametrize("ups", [False, True])
def test_conv_bound_rejects_corrupted_reference(gn, ups):
    from test_vqgan_kernels_gpu import conv_bound

    case = _crossed(gn, ups)
    n, h, w, cin, cout = case[:5]
    d = vr.make_conv_case(case)
    r, a = vr.conv3x3_ref(d["x"], d["w"], d["bias"], d["res"], gn=d["gn"], ups=ups, round_act=True)
    bound = conv_bound(r, a, 9 * cin, gn)
    good = vr.bf16_round(r)  # a correct kernel: one bf16 rounding of the exact result
    assert ((good - r).abs() <= bound).all()

    # (a) tap 0 (dy = dx = -1) dropped for pixels on the image border only
    w_no0 = d["w"].clone()
    w_no0[:, :cin] = 0
    r_no0, _ = vr.conv3x3_ref(d["x"], w_no0, d["bias"], d["res"], gn=d["gn"], ups=ups, round_act=True)
    border = torch.zeros(n, h, w, 1, dtype=torch.bool)
    border[:, [0, -1]] = True
    border[:, :, [0, -1]] = True
    bad = vr.bf16_round(torch.where(border, r_no0, r))
    fails = (bad - r).abs() > bound
    assert fails.any() and not (fails & ~border).any()

    # (b) the GroupNorm table of the neighbouring image
    if gn:
        mean, rstd, gamma, beta = d["gn"]
        rolled = (mean.roll(1, 0), rstd.roll(1, 0), gamma, beta)
        r_sw, _ = vr.conv3x3_ref(d["x"], d["w"], d["bias"], d["res"], gn=rolled, ups=ups, round_act=True)
        assert ((vr.bf16_round(r_sw) - r).abs() > bound).float().mean().item() > 0.5


# ---------------------------------------------------------------------------------------------------------------
# which decoders / code grids the HIP path takes (no GPU needed: the predicates only look at the modules)
def test_hip_decoder_support_predicates():
    from dalle_amd.models.vqgan import Decoder
    from dalle_amd.models.vqgan_hip import grid_supported, supported

    cfg = dict(out_ch=3, ch_mult=(1,), num_res_blocks=1, attn_resolutions=(), resolution=16, z_channels=64)
    dec = Decoder(ch=128, **cfg)
    assert supported(dec)
    dec.mid.block_1.norm2 = torch.nn.GroupNorm(16, 128)  # the kernels hard-code 32 groups
    assert not supported(dec)
    assert not supported(Decoder(ch=96, **cfg))  # channel counts the conv kernel does not tile
    # conv3x3 tiles 128 pixels of one image; the levels only upsample, so the latent grid decides
    assert grid_supported(16, 16) and grid_supported(32, 32) and grid_supported(8, 16)
    assert not grid_supported(8, 8) and not grid_supported(24, 24) and not grid_supported(0, 128)
