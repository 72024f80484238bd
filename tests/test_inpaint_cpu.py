"""Inpainting on the CPU path (``use_hip=False``, fp32): the batched prefill over kept image codes against the same
codes fed step by step, the step window (``prefill_kept`` / ``skip_tail``), the argument checks of the engines and of
``DALLE.generate_images(img_mask=...)``, the pixel-to-cell reduction and a ``serve.py`` request with a picture.

Sampling here is greedy (``top_k=1``): the CPU sampler draws its noise from torch's generator, call by call, so only
greedy runs are comparable bit for bit across calls that run different numbers of steps."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "inference"))

from dalle_amd.config import DALLEConfig, tiny  # noqa: E402
from dalle_amd.data.tokenizer import HashingTokenizer  # noqa: E402
from dalle_amd.models.dalle import DALLE, code_mask  # noqa: E402
from dalle_amd.models.generation import DecodeEngine, SplitDecodeEngine  # noqa: E402

B = 4
CPU = torch.device("cpu")


def _cfg():
    c = tiny(False)
    return DALLEConfig(**{**c.to_dict(), "depth": 4, "attn_types": ["axial_row", "axial_col", "conv_like", "full"],
                          "shared_attn_ids": [0, 1, 2, 3], "shared_ff_ids": [0, 1, 0, 1]})


def suffix_mask(k, L=256):
    return (torch.arange(L) >= k).expand(B, L).clone()


def rect_mask(S=16):
    m = torch.zeros(B, S, S, dtype=torch.bool)
    m[:, 5:10, 3:12] = True  # grid rows 5..9 x cols 3..11: first cell 5 * 16 + 3 = 83, last 9 * 16 + 11 = 155
    return m.reshape(B, S * S)


def per_row_mask(L=256):
    m = torch.zeros(B, L, dtype=torch.bool)
    m[0, 19:] = True
    m[1, 0] = True
    m[2] = True
    m[3, 255] = True
    return m


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(0)
    cfg = _cfg()
    m = DALLE(cfg).eval()
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len))
    tb = m.prepare_text(text)
    image = torch.randint(0, cfg.num_image_tokens, (B, cfg.image_seq_len), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        tf = DecodeEngine(m, B, device=CPU, use_hip=False).teacher_forced_logits(tb, image)
    plain = DecodeEngine(m, B, device=CPU, use_hip=False).generate(tb, top_k=1)
    return cfg, m, text, tb, image, tf, plain


def _eng(m):
    return DecodeEngine(m, B, device=CPU, use_hip=False)


@pytest.mark.parametrize("k0", [1, 16, 17, 32])
def test_kept_prefill_matches_forced_steps(setup, k0):
    """After the batched pass over the caption and k0 kept codes, the KV caches, LN histories, position and next
    input token are what feeding the same codes step by step leaves (k0 % 16 is 1, 0, 1, 0: grid column 0 / 1, in
    the first grid row and below it), nothing is written past P, and the next step's logits agree."""
    cfg, m, text, tb, image, tf, plain = setup
    T = cfg.text_len
    P = T - 1 + k0
    seq, par = _eng(m), _eng(m)
    with torch.no_grad():
        seq.prefill(tb)
        for i in range(k0):  # feed codes 0 .. k0 - 1: the engine ends at position P with code k0 - 1 as its input
            seq._forward_position()
            seq.tok.copy_(image[:, i] + seq.Vt)
            seq.pos.add_(1)
        par.prefill_parallel(tb, kept=image[:, :k0])
        assert int(seq.pos) == int(par.pos) == P and torch.equal(seq.tok, par.tok)
        assert torch.equal(par.codes[:, :k0], image[:, :k0])
        for li in range(len(seq.kc)):
            for a, b in ((seq.kc[li], par.kc[li]), (seq.vc[li], par.vc[li])):
                assert torch.allclose(a[:, :P], b[:, :P], atol=1e-4, rtol=1e-4)
                assert not b[:, P:].any()
            for j in range(2):
                assert torch.allclose(seq.hist[li][j][:, :P], par.hist[li][j][:, :P], atol=1e-4, rtol=1e-4)
                assert not par.hist[li][j][:, P:].any()
        l_seq, l_par = seq._forward_position(), par._forward_position()
    assert torch.allclose(l_seq, l_par, atol=2e-4, rtol=1e-4), (l_seq - l_par).abs().max()
    assert torch.allclose(l_par, tf[:, k0], atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize("k0", [17, 83])
def test_greedy_first_regenerated_code(setup, k0):
    cfg, m, text, tb, image, tf, plain = setup
    out = _eng(m).generate(tb, top_k=1, image=image, regen=suffix_mask(k0))
    assert torch.equal(out[:, :k0], image[:, :k0])
    assert torch.equal(out[:, k0], tf[:, k0].argmax(-1))


def test_rectangle_and_per_row_masks_keep_exactly(setup):
    cfg, m, text, tb, image, tf, plain = setup
    for regen in (rect_mask(), per_row_mask()):
        out = _eng(m).generate(tb, top_k=1, image=image, regen=regen)
        assert torch.equal(out[~regen], image[~regen])
    # the per-row set: row 2 (all True) is an ordinary row, and row 1 differs from it only through its own cell 0
    assert torch.equal(out[2], plain[2])
    # rectangle: the first regenerated code follows the kept picture
    out = _eng(m).generate(tb, top_k=1, image=image, regen=rect_mask())
    assert torch.equal(out[:, 83], tf[:, 83].argmax(-1))


def test_bitwise_equalities(setup):
    cfg, m, text, tb, image, tf, plain = setup
    eng = _eng(m)
    regen = rect_mask()
    a = eng.generate(tb, top_k=1, image=image, regen=regen, skip_tail=True)
    b = eng.generate(tb, top_k=1, image=image, regen=regen, skip_tail=False)
    assert torch.equal(a, b)
    # all True: the unprimed call; all kept: the input; unprimed after masked: a fresh engine's
    assert torch.equal(eng.generate(tb, top_k=1, image=image, regen=torch.ones(B, 256, dtype=torch.bool)), plain)
    assert torch.equal(eng.generate(tb, top_k=1, image=image, regen=torch.zeros(B, 256, dtype=torch.bool)), image)
    assert torch.equal(eng.generate(tb, top_k=1), plain)
    assert not eng.keep.any() and int(eng.n_prime) == 0
    # the prefix mode is the mask i >= k
    k = 19
    assert torch.equal(eng.generate(tb, top_k=1, image=image, regen=suffix_mask(k), prefill_kept=False),
                       eng.generate(tb, top_k=1, prime=image[:, :k]))


def test_split_engine_slices_per_part(setup):
    cfg, m, text, tb, image, tf, plain = setup
    regen = per_row_mask()
    regen[:, :5] = False  # a global k0 of 5 with per-row masks behind it
    single = _eng(m).generate(tb, top_k=1, image=image, regen=regen)
    split = SplitDecodeEngine(m, B, device=CPU, parts=2)
    got = split.generate(tb, top_k=1, image=image, regen=regen)
    assert torch.equal(got[~regen], image[~regen])
    assert (got == single).float().mean().item() > 0.98  # the parts' GEMMs have other row counts
    with pytest.raises(ValueError, match="image"):
        split.generate(tb, top_k=1, image=image[:2], regen=regen)


def test_guided_engine_keeps_both_rows(setup):
    cfg, m, text, tb, image, tf, plain = setup
    regen = rect_mask()
    eng = DecodeEngine(m, B, device=CPU, use_hip=False, guided=True)
    out = eng.generate(tb, top_k=1, image=image, regen=regen, cond_scale=2.0)
    assert torch.equal(out[~regen], image[~regen])
    assert torch.equal(eng.codes[:B], eng.codes[B:])


def test_validation_errors(setup):
    cfg, m, text, tb, image, tf, plain = setup
    eng = _eng(m)
    regen = rect_mask()
    with pytest.raises(ValueError, match="regen"):
        eng.generate(tb, image=image)
    with pytest.raises(ValueError, match="image"):
        eng.generate(tb, regen=regen)
    with pytest.raises(ValueError, match="prime"):
        eng.generate(tb, image=image, regen=regen, prime=image[:, :3])
    with pytest.raises(ValueError, match="image must be"):
        eng.generate(tb, image=image[:, :100], regen=regen)
    with pytest.raises(ValueError, match="regen must be"):
        eng.generate(tb, image=image, regen=regen[:2])
    with pytest.raises(ValueError, match="integer"):
        eng.generate(tb, image=image.float(), regen=regen)
    with pytest.raises(ValueError, match="bool"):
        eng.generate(tb, image=image, regen=regen.long())
    # the public interface
    with pytest.raises(ValueError, match="num_init_img_tokens"):
        m.generate_images(text, img=image, img_mask=regen, num_init_img_tokens=5)
    with pytest.raises(ValueError, match="img_mask needs img"):
        m.generate_images(text, img_mask=regen)
    with pytest.raises(ValueError, match="neither over the codes nor over the pixels"):
        m.generate_images(text, img=image, img_mask=torch.ones(B, 8, 8, dtype=torch.bool))  # neither 16 x 16 nor pixels
    with pytest.raises(ValueError, match="batch size"):
        m.generate_images(text, img=image, img_mask=regen[:2])


def test_generate_images_takes_code_masks(setup):
    cfg, m, text, tb, image, tf, plain = setup
    regen = rect_mask()
    a = m.generate_images(text, img=image, img_mask=regen, top_k=1, return_codes=True)
    b = m.generate_images(text, img=image, img_mask=regen.view(B, 16, 16).to(torch.uint8), top_k=1, return_codes=True)
    assert torch.equal(a, b) and torch.equal(a[~regen], image[~regen])
    assert torch.equal(a, _eng(m).generate(tb, top_k=1, image=image, regen=regen))


def test_pixel_mask_reduces_to_cells():
    """A hand-made pixel mask over a 4 x 4 grid of 8 x 8 cells: one marked pixel marks its cell."""
    g, S = 4, 32
    m = torch.zeros(2, S, S)
    m[0, 0, 0] = 1          # cell (0, 0), its first pixel
    m[0, 15, 23] = 1        # cell (1, 2), its last pixel
    m[1, 8:24, 8:16] = 1    # cells (1, 1) and (2, 1)
    want = torch.zeros(2, g, g, dtype=torch.bool)
    want[0, 0, 0] = want[0, 1, 2] = want[1, 1, 1] = want[1, 2, 1] = True
    assert torch.equal(code_mask(m, 2, g, S), want.view(2, g * g))
    assert torch.equal(code_mask(m.unsqueeze(1), 2, g, S), want.view(2, g * g))
    assert torch.equal(code_mask(want, 2, g, S), want.view(2, g * g))
    assert torch.equal(code_mask(want.view(2, g * g), 2, g), want.view(2, g * g))
    with pytest.raises(ValueError):
        code_mask(m, 2, g)            # pixels without a VAE's image size
    with pytest.raises(ValueError):
        code_mask(m[:, :30, :30], 2, g, S)
    with pytest.raises(ValueError):
        code_mask(m, 3, g, S)


def test_serve_request_with_picture(setup):
    """A request with init_image + mask and one without share a batch: the kept cells are the picture's, and the
    picture-less request's codes are what the same request gives in a batch of picture-less rows."""
    from serve import BatchingGenerator

    cfg, m, text, tb, image, tf, plain = setup
    gen = BatchingGenerator(m, HashingTokenizer(vocab_size=cfg.num_text_tokens), "cpu", max_batch=2, batch_window_ms=5000)
    try:
        regen = rect_mask()[0]
        a = gen.submit(["a red apple"], 1, temperature=0.0)
        b = gen.submit(["a cat"], 1, temperature=0.0, init_image=image[0].tolist(), mask=regen.view(16, 16).tolist())
        ra, rb = a.result(timeout=300), b.result(timeout=300)
        assert ra["batch_images"] == rb["batch_images"] == 2
        got = torch.tensor(rb["codes"][0])
        assert torch.equal(got[~regen], image[0][~regen])
        alone = gen.submit(["a red apple"], 2, temperature=0.0).result(timeout=300)
        assert alone["codes"][0] == ra["codes"][0]
        # a kept prefix through the same door; the argument checks answer in the submitting thread
        c = gen.submit(["a cat"], 2, temperature=0.0, init_image=image[1].tolist(), num_init_img_tokens=7).result(timeout=300)
        assert c["codes"][0][:7] == image[1, :7].tolist()
        with pytest.raises(ValueError, match="init_image"):
            gen.submit(["x"], 1, mask=regen.tolist())
        with pytest.raises(ValueError, match="not both"):
            gen.submit(["x"], 1, init_image=image[0].tolist(), mask=regen.tolist(), num_init_img_tokens=3)
        with pytest.raises(ValueError, match="image codes"):
            gen.submit(["x"], 1, init_image=image[0, :9].tolist())
    finally:
        gen.close()


def test_run_inference_mask_file(tmp_path):
    """``--mask``: white = regenerate, framed like ``--init-image`` (short side resized, centre crop) with nearest
    sampling; it needs ``--init-image`` and excludes ``--num-init-img-tokens`` (checked before anything is loaded)."""
    import numpy as np
    from PIL import Image
    from run_inference import load_mask, main

    a = np.zeros((40, 60), np.uint8)
    a[10:20, 30:50] = 255
    Image.fromarray(a).save(tmp_path / "mask.png")
    m = load_mask(str(tmp_path / "mask.png"), 32)  # 40 x 60 -> 32 x 48 -> columns 8..39
    want = torch.zeros(32, 32, dtype=torch.bool)
    want[8:16, 16:32] = True
    assert m.dtype == torch.bool and torch.equal(m, want)
    base = ["--queries", "q.txt", "--output-dir", str(tmp_path / "out"), "--model-preset", "tiny"]
    with pytest.raises(SystemExit):
        main(base + ["--mask", str(tmp_path / "mask.png")])
    with pytest.raises(SystemExit):
        main(base + ["--mask", str(tmp_path / "mask.png"), "--init-image", "p.png", "--num-init-img-tokens", "5"])
