"""Image-primed generation: forced prefix tokens in the decode engine, ``generate_images(img=,
num_init_img_tokens=)`` and the ``run_inference.generate(init_image=)`` pass-through, on the CPU reference path."""
import os
import sys

import pytest
import torch

from dalle_amd.config import DALLEConfig, tiny
from dalle_amd.models.dalle import DALLE
from dalle_amd.models.generation import DecodeEngine

CPU = torch.device("cpu")


def _cfg(reversible=False):
    c = tiny(reversible)
    return DALLEConfig(**{**c.to_dict(), "depth": 4, "attn_types": ["axial_row", "axial_col", "conv_like", "full"],
                          "shared_attn_ids": [0, 1, 2, 3], "shared_ff_ids": [0, 1, 0, 1]})


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(0)
    cfg = _cfg()
    m = DALLE(cfg).eval()
    B = 2
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len))
    text[:, 30:] = 0
    return cfg, m, B, text, m.prepare_text(text)


def test_forced_prefix_and_first_free_token(setup):
    """codes[:, :k] is the prime, and the first sampled token (greedy) is the argmax of the teacher-forced logits of a
    sequence that starts with the prime: the forced tokens were fed back as input, not only recorded."""
    cfg, m, B, _, tb = setup
    k = 5
    g = torch.Generator().manual_seed(1)
    p = torch.randint(0, cfg.num_image_tokens, (B, k), generator=g)
    eng = DecodeEngine(m, B, device=CPU, use_hip=False)
    codes = eng.generate(tb, prime=p, top_k=1, parallel_prefill=False)
    assert codes.shape == (B, cfg.image_seq_len)
    assert torch.equal(codes[:, :k], p)
    image = torch.randint(0, cfg.num_image_tokens, (B, cfg.image_seq_len), generator=g)
    image[:, :k] = p
    logits = DecodeEngine(m, B, device=CPU, use_hip=False).teacher_forced_logits(tb, image)
    assert torch.equal(codes[:, k], logits[:, k].argmax(-1))
    # the parallel prefill resets the engine once more before the steps: the prefix must survive that too
    again = eng.generate(tb, prime=p, top_k=1)
    assert torch.equal(again[:, :k], p)


def test_empty_prime_changes_nothing(setup):
    cfg, m, B, _, tb = setup
    eng = DecodeEngine(m, B, device=CPU, use_hip=False)

    def run(**kw):
        torch.manual_seed(7)
        return eng.generate(tb, top_k=8, seed=3, parallel_prefill=False, **kw)

    base = run()
    assert torch.equal(run(prime=None), base)
    assert torch.equal(run(prime=torch.zeros(B, 0, dtype=torch.long)), base)
    # ... also right after a primed call on the same engine
    run(prime=torch.ones(B, 4, dtype=torch.long))
    assert torch.equal(run(), base)


def test_prime_validation(setup):
    cfg, m, B, _, tb = setup
    eng = DecodeEngine(m, B, device=CPU, use_hip=False)
    with pytest.raises(ValueError):
        eng.set_prime(torch.zeros(B, cfg.image_seq_len, dtype=torch.long))
    with pytest.raises(ValueError):
        eng.set_prime(torch.zeros(B + 1, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        eng.set_prime(torch.zeros(B, 3))


class _StubVAE(torch.nn.Module):
    """Encodes every picture to codes (row + position) % num_tokens; records what it was given."""

    def __init__(self, n, num_tokens):
        super().__init__()
        self.n, self.num_tokens, self.seen = n, num_tokens, None

    def get_codebook_indices(self, images):
        self.seen = images
        b = images.shape[0]
        return (torch.arange(self.n)[None] + torch.arange(b)[:, None]) % self.num_tokens

    def decode(self, codes):
        return codes


def test_generate_images_priming(setup):
    cfg, m, B, text, _ = setup
    L = cfg.image_seq_len
    codes_in = torch.randint(0, cfg.num_image_tokens, (B, L), generator=torch.Generator().manual_seed(2))
    out = m.generate_images(text, img=codes_in, num_init_img_tokens=6, top_k=4)
    assert out.shape == (B, L) and torch.equal(out[:, :6], codes_in[:, :6])
    # dalle-pytorch's default prefix length
    kd = int(0.4375 * L)
    out = m.generate_images(text, img=codes_in, top_k=4)
    assert torch.equal(out[:, :kd], codes_in[:, :kd])
    with pytest.raises(ValueError):
        m.generate_images(text, img=codes_in, num_init_img_tokens=L)
    with pytest.raises(ValueError):
        m.generate_images(text, img=codes_in[:1], num_init_img_tokens=3)
    pic = torch.rand(B, 3, 8, 8)
    with pytest.raises(ValueError):
        m.generate_images(text, img=pic, num_init_img_tokens=3)  # no VAE
    vae = _StubVAE(L, cfg.num_image_tokens)
    m.vae = vae
    try:
        out = m.generate_images(text, img=pic, num_init_img_tokens=9, top_k=4, return_codes=True)
    finally:
        m.vae = None
    assert vae.seen is pic
    assert torch.equal(out[:, :9], vae.get_codebook_indices(pic)[:, :9])


def test_run_inference_passes_init_image_through():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "inference"))
    try:
        import run_inference
    finally:
        sys.path.pop(0)

    calls = []

    class _Model:
        def generate_images(self, ids, **kw):
            calls.append(kw)
            return torch.zeros(ids.shape[0], 3, 4, 4)

    class _Wrap:
        model = _Model()

    tok = lambda q, **kw: {"input_ids": [5, 6, 7]}  # noqa: E731
    pic = torch.rand(3, 4, 4)
    res = run_inference.generate("q", tokenizer=tok, model=_Wrap(), batch_size=2, n_iters=1, temperature=1.0, top_k=0,
                                 top_p=1.0, text_seq_len=8, device="cpu", init_image=pic, num_init_img_tokens=11)
    assert len(res) == 2
    assert calls[0]["num_init_img_tokens"] == 11
    assert calls[0]["img"].shape == (2, 3, 4, 4) and torch.equal(calls[0]["img"][1], pic)
    run_inference.generate("q", tokenizer=tok, model=_Wrap(), batch_size=2, n_iters=1, temperature=1.0, top_k=0,
                           top_p=1.0, text_seq_len=8, device="cpu")
    assert "img" not in calls[1]


def test_load_init_image_resizes_and_crops(tmp_path):
    from PIL import Image

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "inference"))
    try:
        import run_inference
    finally:
        sys.path.pop(0)
    Image.new("RGB", (40, 24), (255, 0, 0)).save(tmp_path / "p.png")
    t = run_inference.load_init_image(str(tmp_path / "p.png"), 16)
    assert t.shape == (3, 16, 16) and t.dtype == torch.float32
    assert torch.all(t[0] == 1.0) and torch.all(t[1:] == 0.0)
