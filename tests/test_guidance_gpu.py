"""Classifier-free guidance on MI355X: the fused sampler's guided mode (``cond_scale``, ``csrc/kernels/sample.hip``),
the decode attention's per-row text source (``text_src``, ``csrc/kernels/decode.hip``) and the guided decode engines
(eager, hipGraph replay, split) that use both (``models/generation.py``)."""
import copy

import pytest
import torch

from dalle_amd.config import DALLEConfig, tiny
from dalle_amd.models.dalle import DALLE
from dalle_amd.models.generation import DecodeEngine, SplitDecodeEngine, make_decode_engine

pytestmark = pytest.mark.gpu


def _cfg(reversible=False):
    c = tiny(reversible)
    return DALLEConfig(**{**c.to_dict(), "depth": 4, "attn_types": ["axial_row", "axial_col", "conv_like", "full"],
                          "shared_attn_ids": [0, 1, 2, 3], "shared_ff_ids": [0, 1, 0, 1]})


def _C():
    from dalle_amd.ops.hip_ops import C

    return C()


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# -- sampler -------------------------------------------------------------------------------------------------------
def _host_mix(c, u, s):
    """u + s * (c - u) on the host, three separately rounded fp32 operations."""
    c, u = c.cpu(), u.cpu()
    d = c - u
    p = d * torch.tensor(s, dtype=torch.float32)
    return u + p


SAMPLING = [(0, 1.0, 1.0), (16, 1.0, 1.0), (16, 0.9, 1.0), (0, 1.0, 0.0)]  # (top_k, top_p, temperature); last: greedy


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("V", [64, 1000, 8192])  # under one slot per thread, a ragged last slot, the full register set
def test_guided_sample_equals_unguided_on_host_mixed_logits(cuda, V, b):
    C = _C()
    g = torch.Generator().manual_seed(V + b)
    c, u = torch.randn(b, V, generator=g) * 3, torch.randn(b, V, generator=g) * 3
    both = torch.cat([c, u]).to(cuda)
    for scale in (0.0, 1.5, 7.0):
        mixed = _host_mix(c, u, scale).to(cuda)
        st = torch.tensor([scale], dtype=torch.float32, device=cuda)
        for top_k, top_p, temp in SAMPLING:
            for seed, pos in ((1, 0), (5, 3), (2 ** 40 + 7, 70), (9, 318)):
                sd = torch.tensor(seed, dtype=torch.int64, device=cuda)
                want = C.sample_step(mixed, top_k, top_p, temp, sd, _i32(pos, cuda))
                got = C.sample_step(both, top_k, top_p, temp, sd, _i32(pos, cuda), cond_scale=st)
                assert got.shape == (b,)
                assert torch.equal(got, want), (scale, top_k, top_p, temp, seed, pos)
    # u == c: the mix is c at any scale
    same = torch.cat([c, c]).to(cuda)
    sd = torch.tensor(3, dtype=torch.int64, device=cuda)
    for scale in (0.0, 1.5, 7.0):
        st = torch.tensor([scale], dtype=torch.float32, device=cuda)
        assert torch.equal(C.sample_step(same, 16, 0.9, 1.0, sd, _i32(11, cuda), cond_scale=st),
                           C.sample_step(c.to(cuda), 16, 0.9, 1.0, sd, _i32(11, cuda)))


@pytest.mark.parametrize("b", [1, 3])
def test_guided_sample_bookkeeping_writes_both_halves(cuda, b):
    """codes and the next input token for rows r and r + b: during the caption each row's own next caption id (the two
    halves' captions differ), afterwards the picture's code for both; with a prime table the prefix in both halves."""
    C = _C()
    T, img, vt, V, scale = 6, 9, 1000, 1000, 1.5
    g = torch.Generator().manual_seed(b)
    text = torch.randint(2, 900, (2 * b, T), generator=g)
    assert not torch.equal(text[:b], text[b:])
    steps = T + img - 1
    c, u = torch.randn(steps, b, V, generator=g) * 3, torch.randn(steps, b, V, generator=g) * 3
    prime = torch.randint(0, V, (2 * b, img), generator=g).to(cuda)
    text = text.to(cuda)
    seed = torch.tensor(5, dtype=torch.int64, device=cuda)
    st = torch.tensor([scale], dtype=torch.float32, device=cuda)

    def run(guided, n_prime):
        rows = 2 * b if guided else b
        codes = torch.full((rows, img), -1, dtype=torch.int64, device=cuda)
        tok = torch.zeros(rows, dtype=torch.int64, device=cuda)
        kw = {} if n_prime is None else dict(prime=prime[:rows], n_prime=_i32(n_prime, cuda))
        toks, raw = [], []
        for pos in range(steps):
            if guided:
                lg = torch.cat([c[pos], u[pos]]).to(cuda)
                kw["cond_scale"] = st
            else:
                lg = _host_mix(c[pos], u[pos], scale).to(cuda)
            raw.append(C.sample_step(lg, 16, 1.0, 1.0, seed, _i32(pos, cuda), text[:rows], codes, tok, vt, **kw).clone())
            toks.append(tok.clone())
        return codes, torch.stack(toks), torch.stack(raw)

    for n_prime in (None, 3):
        want_codes, want_tok, want_raw = run(False, n_prime)
        codes, toks, raw = run(True, n_prime)
        assert torch.equal(raw, want_raw)
        assert torch.equal(codes[:b], want_codes) and torch.equal(codes[b:], want_codes)
        assert torch.equal(toks[:, :b], want_tok)
        for pos in range(steps):
            exp = text[b:, pos + 1] if pos + 1 < T else raw[pos] + vt
            assert torch.equal(toks[pos, b:], exp), pos
        if n_prime:
            assert torch.equal(codes[:b, :3], prime[:b, :3]) and torch.equal(codes[b:, :3], prime[:b, :3])
            for ci in range(3):
                assert torch.equal(toks[T - 1 + ci, b:], prime[:b, ci] + vt)


def test_guided_sample_argument_checks(cuda):
    C = _C()
    sd, pos = torch.tensor(1, dtype=torch.int64, device=cuda), _i32(0, cuda)
    st = torch.ones(1, dtype=torch.float32, device=cuda)
    lg = torch.randn(4, 64, device=cuda)
    C.sample_step(lg, 0, 1.0, 1.0, sd, pos, cond_scale=st)
    with pytest.raises(RuntimeError):
        C.sample_step(lg[:3].contiguous(), 0, 1.0, 1.0, sd, pos, cond_scale=st)  # odd row count
    with pytest.raises(RuntimeError):
        C.sample_step(lg, 0, 1.0, 1.0, sd, pos, cond_scale=st.double())
    with pytest.raises(RuntimeError):
        C.sample_step(lg, 0, 1.0, 1.0, sd, pos, cond_scale=torch.ones(2, dtype=torch.float32, device=cuda))
    with pytest.raises(RuntimeError):  # every (2 b, ...) operand keeps all rows
        C.sample_step(lg, 0, 1.0, 1.0, sd, pos, torch.zeros(2, 6, dtype=torch.int64, device=cuda),
                      torch.zeros(2, 9, dtype=torch.int64, device=cuda), torch.zeros(2, dtype=torch.int64, device=cuda), 1000,
                      cond_scale=st)


# -- decode attention: per-row text source -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["2", "0"])
def test_text_src_reads_the_source_rows_text_keys_exactly(cuda, mode):
    """Rows 0-1 hold caption A, rows 2-3 caption B: reading the text K / V of rows 1 and 3 from rows 0 and 2 gives
    bitwise the logits of every row reading its own cache (the caches hold the same values)."""
    torch.manual_seed(0)
    cfg = _cfg(False)
    m = DALLE(cfg).eval().to(cuda)
    two = torch.randint(2, cfg.num_text_tokens, (2, cfg.text_seq_len), device=cuda)
    tb = m.prepare_text(two.repeat_interleave(2, 0))
    img = torch.randint(0, cfg.num_image_tokens, (4, cfg.image_seq_len), device=cuda)
    out = []
    for src in ([0, 1, 2, 3], [0, 0, 2, 2]):
        eng = DecodeEngine(m, 4, device=cuda, partials=int(mode))
        eng.text_src = _i32(src, cuda)
        out.append(eng.teacher_forced_logits(tb, img))
        assert int(eng.text_shared.item()) == 0
    assert torch.equal(out[0], out[1])
    # ... and they are the logits of the engine as it was (no text_src, captions not shared)
    assert torch.equal(out[0], DecodeEngine(m, 4, device=cuda, partials=int(mode)).teacher_forced_logits(tb, img))


def test_text_src_argument_checks(cuda):
    torch.manual_seed(0)
    cfg = _cfg(False)
    m = DALLE(cfg).eval().to(cuda)
    eng = DecodeEngine(m, 4, device=cuda)
    C = _C()
    part = torch.zeros(2, 4, 3 * eng.H * 64, dtype=torch.float32, device=cuda)

    def call_part(**kw):
        C.decode_attn_part_(part, eng.cos, eng.sin, 0.125, eng.kc[0], eng.vc[0], eng.obuf, eng.pos, eng.T, eng.S, eng.H,
                            eng.geom.kernel_size, 0, **kw)

    def call(**kw):
        C.decode_attn_(eng.qbuf, eng.kc[0], eng.vc[0], eng.obuf, eng.pos, eng.T, eng.S, eng.H, eng.geom.kernel_size, 0, **kw)

    src = torch.arange(4, dtype=torch.int32, device=cuda)
    for f in (call, call_part):
        f(text_src=src)
        with pytest.raises(RuntimeError):
            f(text_src=src, text_shared=eng.text_shared)
        with pytest.raises(RuntimeError):
            f(text_src=src[:3].contiguous())
        with pytest.raises(RuntimeError):
            f(text_src=src.cpu())
    # entries outside [0, B) are clamped to the batch in the kernel: they read rows 0 and B - 1
    for t in (eng.kc[0], eng.vc[0], eng.qbuf):
        t.copy_(torch.randn(t.shape, device=cuda))
    eng.pos.fill_(5)
    call(text_src=_i32([0, 3, 2, 3], cuda))
    want = eng.obuf.clone()
    eng.obuf.zero_()
    call(text_src=_i32([-7, 100, 2, 3], cuda))
    assert torch.equal(eng.obuf, want)
    call(text_src=src)
    assert not torch.equal(eng.obuf, want)


# -- engines -------------------------------------------------------------------------------------------------------
B = 2


@pytest.fixture(scope="module", params=[False, True], ids=["sequential", "reversible"])
def setup(cuda, request):
    torch.manual_seed(0)
    cfg = _cfg(request.param)
    m = DALLE(cfg).eval().to(cuda)
    text = torch.randint(2, cfg.num_text_tokens, (4, cfg.text_seq_len), device=cuda)
    return cfg, m, m.prepare_text(text)


def test_guided_graph_replay_equals_eager(cuda, setup):
    cfg, m, tb = setup
    eng = DecodeEngine(m, B, device=cuda, guided=True)
    assert eng.fused_sampler and eng.skinny and eng.R == 2 * B
    eager = eng.generate(tb[:B], top_k=16, seed=5, use_graph=False, cond_scale=3.0)
    graph = eng.generate(tb[:B], top_k=16, seed=5, use_graph=True, cond_scale=3.0)
    assert eager.shape == (B, cfg.image_seq_len)
    assert torch.equal(eager, graph)
    assert torch.equal(eng.codes[:B], eng.codes[B:])


def test_one_graph_serves_every_scale_and_prefix(cuda, setup):
    cfg, m, tb = setup
    ref = DecodeEngine(m, B, device=cuda, guided=True)
    want2 = ref.generate(tb[:B], top_k=16, seed=5, use_graph=False, cond_scale=2.0)
    want5 = ref.generate(tb[:B], top_k=16, seed=5, use_graph=False, cond_scale=5.0)
    assert not torch.equal(want2, want5)
    eng = DecodeEngine(m, B, device=cuda, guided=True)
    a = eng.generate(tb[:B], top_k=16, seed=5, use_graph=True, cond_scale=2.0)
    graph = eng.graph
    assert graph is not None
    b = eng.generate(tb[:B], top_k=16, seed=5, use_graph=True, cond_scale=5.0)
    assert eng.graph is graph
    assert torch.equal(a, want2) and torch.equal(b, want5)
    prime = torch.randint(0, cfg.num_image_tokens, (B, 7), generator=torch.Generator().manual_seed(3)).to(cuda)
    c = eng.generate(tb[:B], top_k=16, seed=5, use_graph=True, cond_scale=5.0, prime=prime)
    assert eng.graph is graph
    assert torch.equal(c[:, :7], prime)
    assert torch.equal(c, ref.generate(tb[:B], top_k=16, seed=5, use_graph=False, cond_scale=5.0, prime=prime))


def test_guided_fused_sampler_against_the_torch_step(cuda, setup):
    """Greedy: the fused sampler's mix and the torch fallback's pick the same codes, but for near-ties under bf16
    logits (the bound of the project's other fused-vs-plain comparisons)."""
    cfg, m, tb = setup
    fused = DecodeEngine(m, B, device=cuda, guided=True).generate(tb[:B], top_k=1, seed=5, use_graph=False, cond_scale=2.0)
    plain = DecodeEngine(m, B, device=cuda, guided=True, fused_sampler=False).generate(tb[:B], top_k=1, seed=5,
                                                                                      use_graph=False, cond_scale=2.0)
    assert (plain == fused).float().mean().item() >= 0.98


@pytest.mark.parametrize("captions", ["distinct", "repeated"])
def test_text_src_sharing_changes_nothing(cuda, setup, captions):
    cfg, m, tb = setup
    t = tb[:B] if captions == "distinct" else tb[:1].expand(B, -1).contiguous()
    out = []
    for share in (True, False):
        eng = DecodeEngine(m, B, device=cuda, guided=True)
        eng.share_src = share
        out.append(eng.generate(t, top_k=16, seed=5, cond_scale=3.0))
        src = eng.text_src.tolist()
        if not share:
            assert src == [0, 1, 2, 3]
        else:
            assert src == ([0, 1, 2, 2] if captions == "distinct" else [0, 0, 2, 2])
    assert torch.equal(out[0], out[1])


def test_guided_split_engine_against_single(cuda, setup):
    cfg, m, tb = setup
    single = DecodeEngine(m, 4, device=cuda, guided=True).generate(tb, top_k=1, seed=5, cond_scale=2.0)
    split = SplitDecodeEngine(m, 4, device=cuda, parts=2, guided=True)
    assert all(p.guided and p.B == 2 and p.R == 4 for p in split.parts)
    got = split.generate(tb, top_k=1, seed=5, cond_scale=2.0)
    assert got.shape == single.shape
    assert (got == single).float().mean().item() >= 0.98
    assert int(split.parts[1].seed.item()) == 6  # seeds stay seed + part


def test_engine_factory_decides_parts_on_the_row_count(cuda, setup):
    cfg, m, tb = setup
    assert isinstance(make_decode_engine(m, 16, device=cuda, guided=True), SplitDecodeEngine)  # 32 rows
    assert isinstance(make_decode_engine(m, 16, device=cuda), DecodeEngine)                    # 16 rows
    eng = make_decode_engine(m, 8, device=cuda, guided=True)
    assert isinstance(eng, DecodeEngine) and eng.guided


def test_serving_guided_requests_through_the_guided_graph(cuda):
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "inference"))
    try:
        from serve import BatchingGenerator
    finally:
        sys.path.pop(0)
    from dalle_amd.data.tokenizer import HashingTokenizer

    torch.manual_seed(0)
    cfg = tiny(False)
    model = DALLE(cfg).eval().to(cuda)
    gen = BatchingGenerator(model, HashingTokenizer(vocab_size=cfg.num_text_tokens), cuda, max_batch=8, batch_window_ms=200)
    try:
        futs = [gen.submit([f"prompt {i}"], images_per_prompt=2, temperature=0.0, cond_scale=3.0) for i in range(2)]
        res = [f.result(timeout=100) for f in futs]
        assert all(r["batch_images"] == 4 and r["batch_padded"] == 4 and len(r["codes"]) == 2 for r in res)
        eng = gen.guided_engines[4]
        assert eng.guided and eng.graph is not None and not gen.engines  # captured, and no plain engine built
        graph = eng.graph
        assert res[0]["codes"][0] == res[0]["codes"][1]  # greedy: one prompt, one picture
        other = gen.submit(["prompt 0"], images_per_prompt=4, temperature=0.0, cond_scale=6.0).result(timeout=100)
        assert gen.guided_engines[4] is eng and eng.graph is graph  # another scale: the same engine and graph
        assert float(eng.cond_scale.item()) == 6.0 and len(other["codes"]) == 4
    finally:
        gen.close()


def test_guided_engine_beside_the_plain_one(cuda, setup):
    """An unguided call on a model that also owns a guided engine returns bitwise what a fresh model returns."""
    cfg, m, tb = setup
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len), generator=torch.Generator().manual_seed(4)).to(cuda)
    fresh = copy.deepcopy(m)
    for attr in ("_decode_engine", "_guided_decode_engine"):
        if hasattr(fresh, attr):
            delattr(fresh, attr)
    torch.manual_seed(9)
    want = fresh.generate_images(text, top_k=16)
    torch.manual_seed(9)
    first = m.generate_images(text, top_k=16)
    guided = m.generate_images(text, top_k=16, cond_scale=3.0)
    torch.manual_seed(9)
    again = m.generate_images(text, top_k=16)
    assert torch.equal(first, want) and torch.equal(again, want)
    assert guided.shape == want.shape and m._guided_decode_engine.guided and not m._decode_engine.guided
    with pytest.raises(ValueError):
        m.generate_images(text, top_k=16, cond_scale=-1.0)
