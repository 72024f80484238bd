"""The float64 references of ``tests/vqgan_enc_ref.py`` (what ``test_vqgan_encoder_kernels_gpu.py`` judges the VQGAN
encoder kernels against) agree with ``torch.nn.functional`` in float64; the bf16 operand roundings alone keep the
encoder's latent well inside the bound the GPU test holds the HIP encoder to; and the predicates that decide which
encoders and picture sizes take the HIP path."""
import pytest
import torch
import torch.nn.functional as F

import vqgan_enc_ref as er

TOL = 1e-12  # the float64 tolerance of test_vqgan_ref_cpu.py


def _close(got, want):
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert (got - want).abs().max().item() <= TOL * max(1.0, want.abs().max().item())


def _w_oihw(w, cin):
    return w.double().reshape(w.shape[0], 3, 3, cin).permute(0, 3, 1, 2)


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 4, 6, 32, 8), (1, 2, 8, 64, 4), (3, 8, 2, 16, 5)])
def test_conv_down_ref_is_padded_stride2_conv2d(n, h, w, cin, cout):
    g = torch.Generator().manual_seed(cin + h)
    nn = torch.arange(n, dtype=torch.float64)[:, None, None, None]
    x = (nn + 1) * torch.randn(n, h, w, cin, generator=g, dtype=torch.float64) + 2 * nn
    wk = torch.randn(cout, 9 * cin, generator=g, dtype=torch.float64) / (3 * cin ** 0.5)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    xin = F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1))
    want = F.conv2d(xin, _w_oihw(wk, cin), bias, stride=2).permute(0, 2, 3, 1)
    want_a = F.conv2d(xin.abs(), _w_oihw(wk, cin).abs(), bias.abs(), stride=2).permute(0, 2, 3, 1)
    got, got_a = er.conv_down_ref(x, wk, bias)
    assert got.shape == (n, h // 2, w // 2, cout)
    _close(got, want)
    _close(got_a, want_a)
    got0, _ = er.conv_down_ref(x, wk, None)
    _close(got0, want - bias)


@pytest.mark.parametrize("n,h,w,cout", [(2, 5, 7, 8), (1, 1, 6, 4), (1, 6, 1, 4)])
def test_conv_in_rgb_ref_is_conv2d_of_the_rescaled_image(n, h, w, cout):
    g = torch.Generator().manual_seed(h * w)
    img = torch.rand(n, 3, h, w, generator=g)
    img[0, 0, 0, 0], img[0, 1, -1, -1] = 0.0, 1.0
    wk = torch.randn(cout, 27, generator=g, dtype=torch.float64) / 27 ** 0.5
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    xr = (2 * img - 1).to(torch.bfloat16).double()  # the kernel's contract: bf16(fp32(2 x - 1))
    want = F.conv2d(xr, _w_oihw(wk, 3), bias, padding=1).permute(0, 2, 3, 1)
    want_a = F.conv2d(xr.abs(), _w_oihw(wk, 3).abs(), bias.abs(), padding=1).permute(0, 2, 3, 1)
    got, got_a = er.conv_in_rgb_ref(img, wk, bias)
    _close(got, want)
    _close(got_a, want_a)
    # the rescale is exact at the ends of the range, and within one bf16 rounding of 2 x - 1 elsewhere
    r = er.rgb_rescale(img)
    assert r[0, 0, 0, 0].item() == -1.0 and r[0, 1, -1, -1].item() == 1.0
    assert (r - (2 * img.double() - 1)).abs().max().item() <= 2.0 ** -8


def test_linear_argmax_ref_is_linear():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 24, generator=g, dtype=torch.float64)
    w = torch.randn(13, 24, generator=g, dtype=torch.float64)
    b = torch.randn(13, generator=g, dtype=torch.float64)
    r, a = er.linear_argmax_ref(x, w, b)
    _close(r, F.linear(x, w, b))
    _close(a, F.linear(x.abs(), w.abs(), b.abs()))


def test_plain_vq_argmax_form_is_the_nearest_code():
    """argmin |z - e|^2 = argmax (z . e - |e|^2 / 2): the bias form ``HipEncoder`` hands to ``linear_argmax``."""
    g = torch.Generator().manual_seed(1)
    z = torch.randn(50, 16, generator=g, dtype=torch.float64)
    e = torch.randn(40, 16, generator=g, dtype=torch.float64)
    r, _ = er.linear_argmax_ref(z, e, -0.5 * e.square().sum(1))
    assert torch.equal(r.argmax(1), torch.cdist(z, e).argmin(1))


@pytest.mark.parametrize("is_gumbel", [True, False])
def test_bf16_operand_rounding_alone_stays_under_half_the_latent_bound(is_gumbel):
    """The GPU test holds the HIP encoder's latent to a relative L2 of 5e-2 against the fp32 PyTorch encoder. A
    PyTorch encoder that only rounds every convolution's input and weights to bf16 (fp32 otherwise) stays under half
    of that on the same model and pictures, so the bound leaves room for the kernels' bf16 activations and has not
    been set by what they produce. Measured here: 8.5e-3 (Gumbel and plain VQ share the encoder weights)."""
    vae = er.small_vae(is_gumbel)
    img = er.small_images()
    ref = er.latent(vae, img)
    emu = er.latent_bf16_emulated(vae, img)
    rel = er.rel_l2(emu, ref)
    print(f"bf16-emulated encoder latent, relative L2 vs fp32: {rel:.3e}")
    assert 0 < rel < 0.5 * 5e-2, rel


def test_hip_encoder_support_predicates():
    from dalle_amd.models.vqgan import Encoder, GumbelQuantize
    from dalle_amd.models.vqgan_hip import encoder_grid_supported, supported_encoder

    cfg = dict(ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(), resolution=32, z_channels=128)
    enc = Encoder(ch=128, **cfg)
    qc = torch.nn.Conv2d(128, 64, 1)
    assert supported_encoder(enc) and supported_encoder(enc, qc, GumbelQuantize(256, 64, 64))
    assert supported_encoder(enc, qc, GumbelQuantize(256, 64))                    # plain VQ
    assert not supported_encoder(enc, qc, GumbelQuantize(200, 64, 64))            # code count % 128
    assert not supported_encoder(enc, torch.nn.Conv2d(128, 32, 1), GumbelQuantize(256, 32))  # latent width % 64
    assert not supported_encoder(Encoder(ch=128, double_z=True, **cfg), qc)       # mean / log-variance head
    assert not supported_encoder(Encoder(ch=128, in_channels=1, **cfg))
    assert not supported_encoder(Encoder(ch=96, **cfg))
    enc.mid.block_1.norm2 = torch.nn.GroupNorm(16, 256)
    assert not supported_encoder(enc)
    enc3 = Encoder(ch=128, ch_mult=(1, 2, 4), num_res_blocks=1, attn_resolutions=(), resolution=64, z_channels=128)
    assert encoder_grid_supported(enc3, 64, 64) and encoder_grid_supported(enc3, 32, 128)
    assert not encoder_grid_supported(enc3, 40, 40)   # latent 10 x 10
    assert not encoder_grid_supported(enc3, 66, 64)   # a side the levels cannot halve
    assert not encoder_grid_supported(enc3, 32, 32)   # latent 8 x 8 = 64 pixels
