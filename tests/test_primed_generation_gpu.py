"""Forced prefix tokens on MI355X: the fused sampler's ``prime`` / ``n_prime`` arguments and the decode engines
(eager, hipGraph replay, split engines) that feed them (``csrc/kernels/sample.hip``, ``models/generation.py``)."""
import pytest
import torch

from dalle_amd.config import DALLEConfig, tiny
from dalle_amd.models.dalle import DALLE
from dalle_amd.models.generation import DecodeEngine, SplitDecodeEngine

pytestmark = pytest.mark.gpu


def _cfg(reversible=False):
    c = tiny(reversible)
    return DALLEConfig(**{**c.to_dict(), "depth": 4, "attn_types": ["axial_row", "axial_col", "conv_like", "full"],
                          "shared_attn_ids": [0, 1, 2, 3], "shared_ff_ids": [0, 1, 0, 1]})


B = 4


@pytest.fixture(scope="module")
def setup(cuda):
    torch.manual_seed(0)
    cfg = _cfg()
    m = DALLE(cfg).eval().to(cuda)
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len), device=cuda)
    tb = m.prepare_text(text)
    g = torch.Generator().manual_seed(3)
    primes = {k: torch.randint(0, cfg.num_image_tokens, (B, k), generator=g).to(cuda) for k in (1, 7, 19)}
    return cfg, m, tb, primes


@pytest.mark.parametrize("k", [1, 7])
def test_graph_replay_equals_eager_with_prefix(cuda, setup, k):
    cfg, m, tb, primes = setup
    eng = DecodeEngine(m, B, device=cuda)
    assert eng.fused_sampler
    eager = eng.generate(tb, top_k=16, seed=5, use_graph=False, prime=primes[k])
    graph = eng.generate(tb, top_k=16, seed=5, use_graph=True, prime=primes[k])
    assert torch.equal(eager[:, :k], primes[k]) and torch.equal(graph[:, :k], primes[k])
    assert torch.equal(eager, graph)


def test_one_graph_serves_every_prefix_length(cuda, setup):
    cfg, m, tb, primes = setup
    fresh = DecodeEngine(m, B, device=cuda).generate(tb, top_k=16, seed=5, use_graph=True)
    eng = DecodeEngine(m, B, device=cuda)
    a = eng.generate(tb, top_k=16, seed=5, use_graph=True, prime=primes[7])
    graph = eng.graph
    assert graph is not None and torch.equal(a[:, :7], primes[7])
    b = eng.generate(tb, top_k=16, seed=6, use_graph=True, prime=primes[19])  # 19 crosses an image row (16 wide)
    assert eng.graph is graph
    assert torch.equal(b[:, :19], primes[19])
    # an unprimed call afterwards: nothing of the prefixes is left, bitwise a fresh engine's codes
    c = eng.generate(tb, top_k=16, seed=5, use_graph=True)
    assert eng.graph is graph
    assert torch.equal(c, fresh)


def test_unfused_step_applies_the_same_rule(cuda, setup):
    """The torch fallback of ``_step`` (``fused_sampler=False``) forces the prefix with ``torch.where``; under greedy
    sampling it then continues as the fused engine does."""
    cfg, m, tb, primes = setup
    fused = DecodeEngine(m, B, device=cuda).generate(tb, top_k=1, seed=5, use_graph=False, prime=primes[7])
    plain = DecodeEngine(m, B, device=cuda, fused_sampler=False).generate(tb, top_k=1, seed=5, use_graph=False,
                                                                         prime=primes[7])
    assert torch.equal(plain[:, :7], primes[7])
    assert (plain == fused).float().mean().item() > 0.98


@pytest.mark.parametrize("use_graph", [True])
def test_split_engine_with_prefix(cuda, setup, use_graph):
    cfg, m, tb, primes = setup
    k = 7
    single = DecodeEngine(m, B, device=cuda).generate(tb, top_k=1, use_graph=use_graph, seed=5, prime=primes[k])
    split = SplitDecodeEngine(m, B, device=cuda, parts=2)
    got = split.generate(tb, top_k=1, use_graph=use_graph, seed=5, prime=primes[k])
    assert torch.equal(got[:, :k], primes[k])  # each part took its own rows of the prime
    assert (got == single).float().mean().item() > 0.98
    with pytest.raises(ValueError):
        split.generate(tb, top_k=1, use_graph=use_graph, seed=5, prime=primes[k][:2])


def _C():
    from dalle_amd.ops.hip_ops import C

    return C()


def test_sample_step_prime(cuda):
    Bs, T, img, vt, V = 4, 6, 9, 1000, 64
    g = torch.Generator().manual_seed(0)
    text = torch.randint(2, 900, (Bs, T), generator=g).to(cuda)
    logits = torch.randn(Bs, V, generator=g).to(cuda)
    prime = torch.randint(0, V, (Bs, img), generator=g).to(cuda)
    seed = torch.tensor(5, dtype=torch.int64, device=cuda)
    C = _C()

    def run(n_prime):
        codes = torch.full((Bs, img), -1, dtype=torch.int64, device=cuda)
        tok = torch.zeros(Bs, dtype=torch.int64, device=cuda)
        toks, raw = [], []
        kw = {} if n_prime is None else dict(prime=prime, n_prime=torch.tensor(n_prime, dtype=torch.int32, device=cuda))
        for pos in range(T + img - 1):
            p = torch.tensor(pos, dtype=torch.int32, device=cuda)
            raw.append(C.sample_step(logits, 0, 1.0, 1.0, seed, p, text, codes, tok, vt, **kw).clone())
            toks.append(tok.clone())
        return codes, torch.stack(toks), torch.stack(raw)

    base_codes, base_tok, base_raw = run(None)
    codes, toks, raw = run(3)
    assert torch.equal(codes[:, :3], prime[:, :3])
    assert torch.equal(codes[:, 3:], base_codes[:, 3:])
    # caption positions: untouched; image positions 0..2: the prime's token; afterwards the unprimed run's
    assert torch.equal(toks[:T - 1], base_tok[:T - 1])
    for ci in range(3):
        assert torch.equal(toks[T - 1 + ci], prime[:, ci] + vt)
        assert torch.equal(raw[T - 1 + ci], prime[:, ci])
    assert torch.equal(toks[T + 2:], base_tok[T + 2:]) and torch.equal(raw[T + 2:], base_raw[T + 2:])
    # n_prime = 0 with a table: exactly the unprimed run
    c0, t0, r0 = run(0)
    assert torch.equal(c0, base_codes) and torch.equal(t0, base_tok) and torch.equal(r0, base_raw)
    with pytest.raises(RuntimeError, match="prime"):
        C.sample_step(logits, 0, 1.0, 1.0, seed, torch.tensor(0, dtype=torch.int32, device=cuda), text,
                      torch.zeros(Bs, img, dtype=torch.int64, device=cuda), torch.zeros(Bs, dtype=torch.int64, device=cuda),
                      vt, prime=prime)
