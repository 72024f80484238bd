"""K19: the VQGAN encoder on the hand-written HIP kernels (``HipEncoder``: RGB input conv, ResNet / attention blocks,
stride-2 downsample convs, ``quant_conv`` GEMM, fused projection + argmax) behind ``VQGanVAE.get_codebook_indices``,
against the fp32 PyTorch taming encoder; and the rules that send a call to the PyTorch path instead."""
import pytest
import torch

import vqgan_enc_ref as er

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[True, False], ids=["gumbel", "plain_vq"])
def setup(request, cuda):
    """The small VQGAN of test_vqgan_gpu.py (ch_mult (1, 2, 4), one block per level, attention at 16, resolution 64),
    3 pictures, the fp32 PyTorch latent and codes (computed once)."""
    vae = er.small_vae(request.param).to(cuda)
    img = er.small_images().to(cuda)
    ref_latent = er.latent(vae, img)  # NCHW fp32
    vae.hip_encoder = False
    ref_codes = vae.get_codebook_indices(img)
    vae.hip_encoder = True
    assert vae.use_hip_encoder(64, 64)
    return vae, img, ref_latent, ref_codes


def test_latent_accuracy(setup):
    """Relative L2 of the HipEncoder's pre-quantisation latent against the fp32 PyTorch encoder < 5e-2, the bound the
    whole HIP decoder is held to (bf16 operand roundings alone: 8.5e-3, test_vqgan_enc_ref_cpu.py).
    Measured on MI355X: 1.13e-2 (Gumbel and plain VQ share the encoder weights)."""
    vae, img, ref_latent, _ = setup
    z = vae._hip_encoder.latent(img)
    assert z.dtype == torch.bfloat16 and tuple(z.shape) == (3, 16, 16, 256)
    rel = er.rel_l2(z.permute(0, 3, 1, 2).float().cpu(), ref_latent.cpu())
    print(f"HipEncoder latent, relative L2 vs the fp32 PyTorch encoder: {rel:.3e}")
    assert rel < 5e-2, rel


def test_quantiser_wiring_and_output(setup):
    vae, img, _, ref_codes = setup
    hip = vae._hip_encoder
    codes = vae.get_codebook_indices(img)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (3, 16 * 16)
    assert codes.min() >= 0 and codes.max() < er.N_EMBED
    z = hip.latent(img)
    w, b = hip._selector()
    if vae.quantize.proj is not None:
        assert torch.equal(w, vae.quantize.proj.weight.detach().reshape(er.N_EMBED, -1).bfloat16())
        assert torch.equal(b, vae.quantize.proj.bias.detach().float())
    else:
        cb = vae.codebook.detach().bfloat16()
        assert torch.equal(w, cb) and torch.equal(b, -0.5 * cb.float().square().sum(1))
    direct = hip.C.linear_argmax(z.reshape(-1, z.shape[-1]).contiguous(), w, b).view(3, -1)
    assert torch.equal(codes, direct)
    share = (codes == ref_codes).float().mean().item()
    print(f"codes equal to the fp32 PyTorch codes: {share:.4f} (random weights: near-ties are common; not asserted)")


def test_fallback_rules(setup, monkeypatch):
    """gumbel_tau > 0 (Gumbel models), a 40 x 40 picture and hip_encoder = False each run the PyTorch path: the latent
    that path computes equals a second PyTorch run within 1e-5, and the cached HipEncoder survives."""
    vae, img, ref_latent, ref_codes = setup
    hip = vae._hip_encoder
    seen = []
    quant_conv_forward = vae.quant_conv.forward

    def spy(x):
        y = quant_conv_forward(x)
        seen.append(y)
        return y

    monkeypatch.setattr(vae.quant_conv, "forward", spy)
    vae.get_codebook_indices(img)
    assert not seen  # the HIP path does not go through the torch modules

    def torch_latent_of_call(fn):
        seen.clear()
        out = fn()
        assert len(seen) == 1, "the PyTorch path ran"
        return out, seen[0]

    if vae.quantize.proj is not None:
        g = torch.Generator(device=img.device).manual_seed(3)
        out, lat = torch_latent_of_call(lambda: vae.get_codebook_indices(img, gumbel_tau=1.0, generator=g))
        assert (lat - ref_latent).abs().max().item() <= 1e-5 and out.shape == ref_codes.shape
    small = er.small_images(2, 40).to(img.device)
    assert not vae.use_hip_encoder(40, 40)
    out, lat = torch_latent_of_call(lambda: vae.get_codebook_indices(small))
    seen_lat = lat
    monkeypatch.undo()
    assert (seen_lat - er.latent(vae, small)).abs().max().item() <= 1e-5 and tuple(out.shape) == (2, 100)
    monkeypatch.setattr(vae.quant_conv, "forward", spy)
    monkeypatch.setattr(vae, "hip_encoder", False)
    out, lat = torch_latent_of_call(lambda: vae.get_codebook_indices(img))
    assert (lat - ref_latent).abs().max().item() <= 1e-5
    monkeypatch.undo()
    assert vae._hip_encoder is hip and vae.use_hip_encoder(64, 64)
    assert torch.equal(vae.get_codebook_indices(img), hip(img))


def test_cpu_images_take_the_pytorch_path(setup):
    vae, img, _, ref_codes = setup
    cpu = er.small_vae(vae.quantize.proj is not None)
    codes = cpu.get_codebook_indices(img.cpu())
    assert getattr(cpu, "_hip_encoder", None) is None and codes.shape == ref_codes.shape
