"""Per-picture sampling parameters on the CPU path: ``filter_logits_rows`` against ``filter_logits``, the torch step of
a row-parameter engine (greedy rows, per-row generators), the host-side validation and ``DALLE.generate_images``."""
import pytest
import torch

from dalle_amd.config import tiny
from dalle_amd.models.dalle import DALLE
from dalle_amd.models.generation import (DecodeEngine, SplitDecodeEngine, filter_logits, filter_logits_rows,
                                         make_decode_engine, row_generator_seed)

B = 4


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("V", [37, 1000])
def test_filter_logits_rows(V, quantised):
    torch.manual_seed(V)
    params = [(0, 1.0), (1, 1.0), (256, 1.0), (0, 0.9), (64, 0.5), (0, 1.0), (V, 0.95), (V + 5, 1e-6)]
    logits = torch.randn(len(params), V) * 3
    if quantised:  # 8 distinct values: ties at the k-th value and at the nucleus cut
        logits = (logits.clamp(-4, 3.99) + 4).floor() - 4
    got = filter_logits_rows(logits, torch.tensor([p[0] for p in params]), torch.tensor([p[1] for p in params]))
    for r, (k, p) in enumerate(params):
        assert torch.equal(got[r], filter_logits(logits[r:r + 1], k, p)[0]), (r, k, p)
    assert torch.isfinite(got).any(-1).all()


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(0)
    cfg = tiny(False)
    m = DALLE(cfg).eval()
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len))
    return cfg, m, text, m.prepare_text(text)


def test_cpu_engine_rows(setup):
    cfg, m, text, tb = setup
    greedy = DecodeEngine(m, B).generate(tb, temperature=0.0, seed=1)
    eng = DecodeEngine(m, B, row_params=True)
    assert not eng.use_hip and not eng.fused_sampler
    kw = {"temperature": [0.0, 1.0, 1.0, 0.8], "top_k": [0, 1, 0, 32], "top_p": [1.0, 1.0, 0.9, 1.0]}
    a = eng.generate(tb, seed=[1, 2, 3, 4], **kw)
    assert torch.equal(a[0], greedy[0]) and torch.equal(a[1], greedy[1])  # temperature 0, and top_k = 1
    # row 2 keeps its draws when its neighbours' parameters and seeds change ...
    b = eng.generate(tb, temperature=[1.0, 0.5, 1.0, 0.0], top_k=[9, 0, 0, 0], top_p=[1.0, 0.5, 0.9, 1.0], seed=[7, 8, 3, 9])
    assert torch.equal(b[2], a[2]) and not torch.equal(b[0], a[0])
    # ... and loses them with its own seed or noise row
    c = eng.generate(tb, seed=[1, 2, 33, 4], **kw)
    d = eng.generate(tb, seed=[1, 2, 3, 4], noise_row=[0, 1, 5, 3], **kw)
    assert not torch.equal(c[2], a[2]) and not torch.equal(d[2], a[2])
    assert torch.equal(c[3], a[3]) and torch.equal(d[3], a[3])
    assert torch.equal(eng.generate(tb, seed=[1, 2, 3, 4], **kw), a)
    assert row_generator_seed(3, 2) == 3 * 2 ** 24 + 2 and row_generator_seed(-1, 0) == 2 ** 63 - 2 ** 24


def test_cpu_guided_rows(setup):
    cfg, m, text, tb = setup
    eng = DecodeEngine(m, B, guided=True, row_params=True)
    plain = DecodeEngine(m, B, guided=True)
    got = eng.generate(tb, temperature=0.0, cond_scale=[0.0, 1.0, 3.0, 1.0])
    for j, s in enumerate([0.0, 1.0, 3.0, 1.0]):
        assert torch.equal(got[j], plain.generate(tb, temperature=0.0, cond_scale=s)[j]), j


def test_validation(setup):
    cfg, m, text, tb = setup
    eng = DecodeEngine(m, B, row_params=True)
    guided = DecodeEngine(m, B, guided=True, row_params=True)
    launched = []
    for e in (eng, guided):
        e._start = lambda *a, **k: launched.append(1)  # nothing may start before the checks are through
    for kw in ({"temperature": [1.0] * 3}, {"top_k": [1] * 5}, {"top_p": (0.5, 0.5)}, {"seed": torch.arange(3)},
               {"noise_row": [0, 1]}):
        with pytest.raises(ValueError, match="one entry per picture"):
            eng.generate(tb, **kw)
    with pytest.raises(ValueError, match="cond_scale must be >= 0"):
        guided.generate(tb, cond_scale=[1.0, 2.0, -0.5, 1.0])
    with pytest.raises(ValueError, match="one entry per picture"):
        guided.generate(tb, cond_scale=[1.0, 2.0])
    with pytest.raises(ValueError, match="guided=True"):
        eng.generate(tb, cond_scale=[1.0] * B)
    for bad in ([0, 1, 2, 2 ** 24], [0, -1, 2, 3]):
        with pytest.raises(ValueError, match="noise_row"):
            eng.generate(tb, noise_row=bad)
    for bad in (float("nan"), [0.5, float("inf"), 0.5, 0.5]):
        with pytest.raises(ValueError, match="top_p must be finite"):
            eng.generate(tb, top_p=bad)
    with pytest.raises(ValueError, match="64 bits"):
        eng.generate(tb, seed=2 ** 63)
    assert not launched
    for plain in (DecodeEngine(m, B), SplitDecodeEngine(m, B, parts=2), make_decode_engine(m, B)):
        for kw in ({"temperature": [1.0] * B}, {"top_k": (1,) * B}, {"top_p": torch.ones(B)}, {"seed": [1] * B},
                   {"noise_row": list(range(B))}):
            with pytest.raises(ValueError, match="row_params=True"):
                plain.generate(tb, **kw)
    assert make_decode_engine(m, B, row_params=True).row_params


def test_split_engine_slices_the_tables(setup):
    cfg, m, text, tb = setup
    kw = {"temperature": [1.0, 0.7, 1.0, 0.9], "top_k": [0, 16, 0, 1], "top_p": [0.9, 1.0, 1.0, 1.0], "seed": [4, 5, 6, 7]}
    one = DecodeEngine(m, B, row_params=True).generate(tb, **kw)
    split = SplitDecodeEngine(m, B, parts=2, row_params=True)
    assert torch.equal(split.generate(tb, **kw), one)  # fp32 on the CPU: the parts compute what the whole batch does
    assert split.parts[1].noise_row.tolist() == [2, 3] and split.parts[1].row_seed.tolist() == [6, 7]


def test_generate_images(setup):
    cfg, m, text, tb = setup
    m = DALLE(cfg).eval()
    m.load_state_dict(setup[1].state_dict())
    # the plain path hands a scalar seed to the plain engine (whose torch step, here, draws from the global generator:
    # the seed keys the fused sampler's noise; tests/test_row_sampling_gpu.py replays it)
    a = m.generate_images(text, seed=11, top_k=16)
    plain = m._decode_engine
    assert not plain.row_params and getattr(m, "_row_decode_engine", None) is None
    seen = {}
    real = plain.generate
    plain.generate = lambda *args, **kw: seen.update(kw) or real(*args, **kw)
    m.generate_images(text, seed=11, top_k=16)
    assert seen["seed"] == 11 and "noise_row" not in seen
    seen.clear()
    m.generate_images(text, top_k=16)
    assert "seed" not in seen
    plain.generate = real
    # a scalar seed on the row path: called twice, the same codes
    r1 = m.generate_images(text, seed=11, top_k=16, noise_row=list(range(B)))
    assert torch.equal(m.generate_images(text, seed=11, top_k=16, noise_row=list(range(B))), r1)
    assert not torch.equal(m.generate_images(text, seed=12, top_k=16, noise_row=list(range(B))), r1)
    lists = m.generate_images(text, temperature=[1.0, 0.5, 1.0, 0.0], top_k=(0, 8, 0, 0), top_p=torch.tensor([1.0, 1.0, 0.8, 1.0]),
                              seed=[1, 2, 3, 4])
    assert lists.shape == a.shape and m._row_decode_engine.row_params and not m._row_decode_engine.guided
    again = m.generate_images(text, temperature=(1.0, 0.5, 1.0, 0.0), top_k=torch.tensor([0, 8, 0, 0]), top_p=[1.0, 1.0, 0.8, 1.0],
                              seed=torch.tensor([1, 2, 3, 4]), noise_row=[0, 1, 2, 3])
    assert torch.equal(again, lists)
    assert m._decode_engine is plain
    g = m.generate_images(text, cond_scale=[1.0, 2.0, 1.0, 0.0], seed=3)
    assert g.shape == a.shape and m._guided_row_decode_engine.guided and m._guided_row_decode_engine.row_params
    assert getattr(m, "_guided_decode_engine", None) is None
    m.generate_images(text, cond_scale=[1.0] * B, seed=3)  # all ones: not guided
    assert m.generate_images(text, noise_row=[3, 2, 1, 0], seed=3).shape == a.shape
    with pytest.raises(ValueError, match="cond_scale must be >= 0"):
        m.generate_images(text, cond_scale=[1.0, -1.0, 1.0, 1.0])


def test_run_inference_seed_rule():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "inference"))
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
    common = dict(tokenizer=tok, model=_Wrap(), batch_size=2, n_iters=3, temperature=1.0, top_k=0, top_p=1.0,
                  text_seq_len=8, device="cpu")
    run_inference.generate("q", seed=40, query_index=2, **common)
    assert [c["seed"] for c in calls] == [40 + 2 * 1000003 + i for i in range(3)]
    assert run_inference.call_seed(2 ** 62 - 1, 0, 1) == 0
    calls.clear()
    run_inference.generate("q", **common)
    assert all("seed" not in c for c in calls)
