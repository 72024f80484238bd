"""Classifier-free guidance on the CPU reference path: ``DALLE.forward(null_cond_prob=)`` (caption dropout), guided
decode engines (two rows per picture, sampled from ``u + s * (c - u)``), ``generate_images(cond_scale=)`` and the
pass-through of both knobs in the trainer arguments, ``run_inference.generate`` and the serving front-end."""
import os
import sys

import pytest
import torch

from dalle_amd.config import DALLEConfig, tiny
from dalle_amd.models.dalle import DALLE
from dalle_amd.models.generation import DecodeEngine

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    image = torch.randint(0, cfg.num_image_tokens, (B, cfg.image_seq_len))
    return cfg, m, B, text, image


# -- training: null_cond_prob --------------------------------------------------------------------------------------
def test_null_cond_prob_zero_is_the_plain_forward(setup):
    cfg, m, B, text, image = setup
    base = m(text, image, return_loss=True)
    state = torch.get_rng_state()
    got = m(text, image, return_loss=True, null_cond_prob=0.0)
    assert torch.equal(got, base)
    assert torch.equal(torch.get_rng_state(), state)  # no random numbers drawn: existing seeds reproduce


def test_null_cond_prob_one_is_the_null_caption(setup):
    cfg, m, B, text, image = setup
    assert torch.equal(m(text, image, return_loss=True, null_cond_prob=1.0),
                       m(torch.zeros_like(text), image, return_loss=True))


def test_null_cond_prob_half_drops_rows_of_the_seeded_mask(setup):
    cfg, m, _, _, _ = setup
    B = 8
    g0 = torch.Generator().manual_seed(11)
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len), generator=g0)
    image = torch.randint(0, cfg.num_image_tokens, (B, cfg.image_seq_len), generator=g0)
    mask = torch.rand(B, generator=torch.Generator().manual_seed(5)) < 0.5
    assert 0 < int(mask.sum()) < B  # the seed drops some rows and keeps some
    dropped = text.clone()
    dropped[mask] = 0
    got = m(text, image, return_loss=True, null_cond_prob=0.5, generator=torch.Generator().manual_seed(5))
    assert torch.equal(got, m(dropped, image, return_loss=True))
    assert not torch.equal(got, m(text, image, return_loss=True))


@pytest.mark.parametrize("p", [-0.1, 1.5])
def test_null_cond_prob_out_of_range_raises(setup, p):
    cfg, m, B, text, image = setup
    with pytest.raises(ValueError):
        m(text, image, return_loss=True, null_cond_prob=p)


# -- guided decode engine ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parallel_prefill", [False, True])
def test_guided_engine_samples_from_the_mixed_logits(setup, parallel_prefill):
    """Greedy: the first code is the argmax of u + s * (c - u) of the teacher-forced logits of the caption (c) and of
    the null caption (u); the second is the argmax of the mix after BOTH streams were fed the first code."""
    cfg, m, B, text, _ = setup
    s = 3.0
    tb = m.prepare_text(text)
    null = m.prepare_text(torch.zeros_like(text))
    eng = DecodeEngine(m, B, device=CPU, use_hip=False, guided=True)
    assert eng.B == B and eng.R == 2 * B and eng.kc[0].shape[0] == 2 * B * cfg.heads
    codes = eng.generate(tb, top_k=1, cond_scale=s, parallel_prefill=parallel_prefill)
    assert codes.shape == (B, cfg.image_seq_len)
    assert torch.equal(eng.codes[:B], eng.codes[B:])  # both halves recorded the pictures' codes

    def mixed(image):
        c = DecodeEngine(m, B, device=CPU, use_hip=False).teacher_forced_logits(tb, image)
        u = DecodeEngine(m, B, device=CPU, use_hip=False).teacher_forced_logits(null, image)
        return u + s * (c - u), c

    image = torch.zeros(B, cfg.image_seq_len, dtype=torch.long)
    mix, c = mixed(image)
    first = mix[:, 0].argmax(-1)
    assert torch.equal(codes[:, 0], first)
    assert not torch.equal(first, c[:, 0].argmax(-1))  # the guidance decided it, not the conditional stream alone
    image[:, 0] = first
    assert torch.equal(codes[:, 1], mixed(image)[0][:, 1].argmax(-1))


def test_guided_engine_scale_validation(setup):
    cfg, m, B, text, _ = setup
    tb = m.prepare_text(text)
    eng = DecodeEngine(m, B, device=CPU, use_hip=False, guided=True)
    with pytest.raises(ValueError):
        eng.generate(tb, top_k=1, cond_scale=-1.0)
    with pytest.raises(ValueError):
        DecodeEngine(m, B, device=CPU, use_hip=False).generate(tb, top_k=1, cond_scale=2.0)  # not a guided engine


# -- generate_images -----------------------------------------------------------------------------------------------
def test_generate_images_scale_one_is_the_unguided_path(setup):
    cfg, m, B, text, _ = setup

    def run(**kw):
        torch.manual_seed(7)
        return m.generate_images(text, top_k=8, **kw)

    base = run()
    assert torch.equal(run(cond_scale=1.0), base)
    assert getattr(m, "_guided_decode_engine", None) is None  # no guided engine was built for it


def test_generate_images_guided_keeps_the_forced_prefix_and_caches_both_engines(setup):
    cfg, m, B, text, _ = setup
    L = cfg.image_seq_len
    codes_in = torch.randint(0, cfg.num_image_tokens, (B, L), generator=torch.Generator().manual_seed(2))
    torch.manual_seed(7)
    base = m.generate_images(text, top_k=8)
    plain_eng = m._decode_engine
    out = m.generate_images(text, img=codes_in, num_init_img_tokens=6, top_k=4, cond_scale=3.0)
    assert out.shape == (B, L) and torch.equal(out[:, :6], codes_in[:, :6])
    guided_eng = m._guided_decode_engine
    assert guided_eng.guided and guided_eng.B == B
    # alternating calls rebuild neither engine, and the plain path still gives what it gave
    torch.manual_seed(7)
    assert torch.equal(m.generate_images(text, top_k=8), base)
    m.generate_images(text, top_k=4, cond_scale=2.0)
    assert m._decode_engine is plain_eng and m._guided_decode_engine is guided_eng


def test_generate_images_negative_scale_raises(setup):
    cfg, m, B, text, _ = setup
    with pytest.raises(ValueError):
        m.generate_images(text, top_k=4, cond_scale=-0.5)


# -- pass-through --------------------------------------------------------------------------------------------------
def _inference_module(name):
    sys.path.insert(0, os.path.join(ROOT, "inference"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_run_inference_passes_cond_scale_through():
    run_inference = _inference_module("run_inference")
    calls = []

    class _Model:
        def generate_images(self, ids, **kw):
            calls.append(kw)
            return torch.zeros(ids.shape[0], 3, 4, 4)

    class _Wrap:
        model = _Model()

    tok = lambda q, **kw: {"input_ids": [5, 6, 7]}  # noqa: E731
    common = dict(tokenizer=tok, model=_Wrap(), batch_size=2, n_iters=1, temperature=1.0, top_k=0, top_p=1.0,
                  text_seq_len=8, device="cpu")
    run_inference.generate("q", cond_scale=3.0, **common)
    assert calls[0]["cond_scale"] == 3.0
    run_inference.generate("q", **common)
    assert calls[1].get("cond_scale", 1.0) == 1.0


def test_server_batches_by_guidance_scale():
    serve = _inference_module("serve")
    torch.manual_seed(0)
    c = tiny(False)
    cfg = DALLEConfig(**{**c.to_dict(), "text_seq_len": 16, "image_size": 64})  # 8x8 codes: fast on CPU
    model = DALLE(cfg).eval()
    from dalle_amd.data.tokenizer import HashingTokenizer

    gen = serve.BatchingGenerator(model, HashingTokenizer(vocab_size=cfg.num_text_tokens), "cpu", max_batch=8,
                                  batch_window_ms=300)
    try:
        a = gen.submit(["a red apple"], temperature=0.0, cond_scale=3.0)
        b = gen.submit(["a cat"], temperature=0.0, cond_scale=3.0)
        c2 = gen.submit(["a cat"], temperature=0.0, cond_scale=5.0)
        ra, rb, rc = a.result(timeout=300), b.result(timeout=300), c2.result(timeout=300)
        assert ra["batch_images"] == rb["batch_images"] == 2  # same scale: one batch
        assert rc["batch_images"] == 1                        # another scale: its own batch
        # guided engines are cached by padded picture count, beside (not among) the plain ones
        assert sorted(gen.guided_engines) == [1, 2] and not gen.engines
        assert all(e.guided for e in gen.guided_engines.values())
        with pytest.raises(ValueError):
            gen.submit(["x"], cond_scale=-1.0)
    finally:
        gen.close()
    if serve.GenerateRequest is not None:
        assert serve.GenerateRequest(prompts=["x"]).cond_scale == 1.0
        assert serve.GenerateRequest(prompts=["x"], cond_scale=3).cond_scale == 3.0
        with pytest.raises(Exception):
            serve.GenerateRequest(prompts=["x"], cond_scale=-1)


def test_null_cond_prob_flag_reaches_the_model_wrapper(tmp_path):
    sys.path.insert(0, ROOT)
    from arguments import CollaborativeArguments, HFTrainerArguments, TrainingPeerArguments
    from dalle_amd.utils.argparse import HfArgumentParser
    from task import TrainingTask

    parser = HfArgumentParser((TrainingPeerArguments, HFTrainerArguments, CollaborativeArguments))
    peer, tr, collab = parser.parse_args_into_dataclasses(
        ["--null_cond_prob", "0.25", "--model_preset", "tiny", "--text_seq_length", "64", "--authorize", "False",
         "--output_dir", str(tmp_path / "out"), "--state_path", str(tmp_path / "state.zip")])
    assert tr.null_cond_prob == 0.25
    assert HFTrainerArguments().null_cond_prob == 0.0
    wrapper = TrainingTask(peer, tr, collab).model
    assert wrapper.null_cond_prob == 0.25
    seen = {}

    class _Spy(torch.nn.Module):
        def forward(self, **kw):
            seen.update(kw)
            return torch.zeros(())

    wrapper.model = _Spy()
    wrapper.train()
    wrapper(input_ids=torch.zeros(1, 64, dtype=torch.long), attention_mask=None, image=None)
    assert seen["null_cond_prob"] == 0.25
    seen.clear()
    wrapper.eval()  # evaluation runs on the captions as given
    wrapper(input_ids=torch.zeros(1, 64, dtype=torch.long), attention_mask=None, image=None)
    assert "null_cond_prob" not in seen
