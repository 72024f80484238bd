"""Per-picture sampling parameters on MI355X: the ``ROWS`` instantiations of the fused sampler
(``csrc/kernels/sample.hip``) against the scalar kernel, row by row and bit for bit, and the row-parameter decode
engines (``models/generation.py``) against the plain ones: the four exactness contracts of the README's
"Per-picture sampling parameters" paragraph."""
import pytest
import torch

from dalle_amd.config import tiny
from dalle_amd.models.dalle import DALLE
from dalle_amd.models.generation import DecodeEngine, SplitDecodeEngine, filter_logits

pytestmark = pytest.mark.gpu

B = 4


def _C():
    from dalle_amd.ops.hip_ops import C

    return C()


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _i64(v, dev):
    return torch.tensor(v, dtype=torch.int64, device=dev)


def _f32(v, dev):
    return torch.tensor(v, dtype=torch.float32, device=dev)


def _tables(params, seeds, dev, noise_row=None):
    """params: one (top_k, top_p, temperature) per row."""
    kw = {"row_top_k": _i32([p[0] for p in params], dev), "row_top_p": _f32([p[1] for p in params], dev),
          "row_temperature": _f32([p[2] for p in params], dev), "row_seed": _i64(list(seeds), dev)}
    if noise_row is not None:
        kw["noise_row"] = _i32(list(noise_row), dev)
    return kw


def _params(V):
    return [(0, 1.0, 1.0), (1, 1.0, 1.0), (256, 1.0, 1.0), (0, 0.9, 1.0), (64, 0.5, 0.7), (0, 1.0, 0.0), (V, 0.95, 1.0),
            (V + 5, 1e-6, 1.3)]


SEEDS = [11, 2 ** 40 + 3, 7, 123456789, 5, 2 ** 62 - 1, 99, 31337]


# -- kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("V", [8192, 1000, 37])
def test_row_equals_scalar(cuda, V, quantised):
    torch.manual_seed(V)
    logits = torch.randn(8, V, device=cuda) * 3
    if quantised:  # 8 distinct values: heavy ties at the k-th value and at the nucleus cut
        logits = (logits.clamp(-4, 3.99) + 4).floor() - 4
    params, C = _params(V), _C()
    dummy = _i64(0, cuda)
    for pos in (0, 5, 300):
        p = _i32(pos, cuda)
        got = C.sample_step(logits, 0, 1.0, 1.0, dummy, p, **_tables(params, SEEDS, cuda))
        for r, ((k, tp, t), s) in enumerate(zip(params, SEEDS)):
            want = C.sample_step(logits, k, tp, t, _i64(s, cuda), p)
            assert got[r].item() == want[r].item(), (V, pos, r, params[r])
    # the scalar arguments are not read with tables, and an explicit arange is the default
    again = C.sample_step(logits, 3, 0.2, 0.0, _i64(77, cuda), p, **_tables(params, SEEDS, cuda, noise_row=range(8)))
    assert torch.equal(again, got)


def test_rows_stay_in_their_filtered_sets(cuda):
    """The inputs of test_sampler_gpu.py::test_samples_stay_in_the_filtered_set, one (top_k, top_p) pair per row."""
    torch.manual_seed(0)
    n, V = 16, 8192
    logits = torch.randn(n, V, device=cuda) * 3
    pairs = [(0, 1.0), (256, 1.0), (1, 1.0), (0, 0.9), (256, 0.8), (50, 0.3), (8192, 0.95)]
    rows = [pairs[r % len(pairs)] for r in range(n)]
    kept = torch.cat([torch.isfinite(filter_logits(logits[r:r + 1], *rows[r])) for r in range(n)])
    C, p, dummy = _C(), _i32(0, cuda), _i64(0, cuda)
    for t in range(20):
        nxt = C.sample_step(logits, 0, 1.0, 1.0, dummy, p,
                            **_tables([(k, tp, 1.0) for k, tp in rows], [t * n + r for r in range(n)], cuda))
        assert nxt.dtype == torch.int64 and nxt.shape == (n,)
        assert kept.gather(1, nxt.view(n, 1)).all(), t
    g = C.sample_step(logits, 0, 1.0, 1.0, dummy, p, **_tables([(k, tp, 0.0) for k, tp in rows], [123] * n, cuda))
    assert torch.equal(g, logits.argmax(-1))


def test_noise_row(cuda):
    torch.manual_seed(1)
    V, C = 1000, _C()
    logits = (torch.randn(V, device=cuda) * 2).repeat(8, 1)
    p, seed = _i32(9, cuda), 4242
    scalar = C.sample_step(logits, 64, 0.9, 1.1, _i64(seed, cuda), p)
    assert len(set(scalar.tolist())) > 1  # the rows do draw different noise
    same = C.sample_step(logits, 0, 1.0, 1.0, _i64(0, cuda), p, **_tables([(64, 0.9, 1.1)] * 8, [seed] * 8, cuda, noise_row=[3] * 8))
    assert (same == scalar[3]).all()
    perm = [5, 2, 7, 0, 1, 6, 3, 4]
    got = C.sample_step(logits, 0, 1.0, 1.0, _i64(0, cuda), p, **_tables([(64, 0.9, 1.1)] * 8, [seed] * 8, cuda, noise_row=perm))
    assert torch.equal(got, scalar[perm])
    # only 24 bits of the entry reach the key
    high = C.sample_step(logits, 0, 1.0, 1.0, _i64(0, cuda), p,
                         **_tables([(64, 0.9, 1.1)] * 8, [seed] * 8, cuda, noise_row=[v + (1 << 24) for v in perm]))
    assert torch.equal(high, got)


@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (5, 1.0), (0, 0.7)])
def test_row_sampling_distribution(cuda, top_k, top_p):
    """test_sampler_gpu.py::test_sampling_distribution through the tables: same setting, same number of draws."""
    V, n = 16, 8192
    base = torch.linspace(-2.0, 1.5, V, device=cuda)
    logits = base.repeat(n, 1)
    temperature = 0.8
    want = torch.softmax(filter_logits(base.view(1, V), top_k, top_p) / temperature, -1).view(V)
    got = torch.zeros(V, device=cuda)
    kw = {"row_top_k": torch.full((n,), top_k, dtype=torch.int32, device=cuda),
          "row_top_p": torch.full((n,), top_p, dtype=torch.float32, device=cuda),
          "row_temperature": torch.full((n,), temperature, dtype=torch.float32, device=cuda),
          "noise_row": torch.arange(n, dtype=torch.int32, device=cuda)}
    for seed in range(4):
        nxt = _C().sample_step(logits, 0, 1.0, 1.0, _i64(0, cuda), _i32(0, cuda),
                               row_seed=torch.full((n,), 1000 + seed, dtype=torch.int64, device=cuda), **kw)
        got += torch.bincount(nxt, minlength=V).float()
    got /= got.sum()
    assert (got[want == 0] == 0).all()
    assert (got - want).abs().max().item() < 0.015, (got, want)


MIXED = [(0, 1.0, 1.0), (8, 1.0, 0.7), (0, 0.8, 1.0), (0, 1.0, 0.0)]
MIXED_SEEDS = [5, 6, 2 ** 33, 8]


@pytest.mark.parametrize("mode", ["plain", "prime", "keep"])
def test_bookkeeping(cuda, mode):
    T, img, vt, V, C = 6, 9, 1000, 64, _C()
    g = torch.Generator().manual_seed(2)
    text = torch.randint(2, 900, (B, T), generator=g).to(cuda)
    prime = torch.randint(0, V, (B, img), generator=g).to(cuda)
    keep = (torch.rand(B, img, generator=g) < 0.4).to(torch.uint8).to(cuda)
    logits = [torch.randn(B, V, generator=g).to(cuda) for _ in range(T + img - 1)]
    kw = {}
    if mode != "plain":
        kw = {"prime": prime, "n_prime": _i32(3, cuda)}
    if mode == "keep":
        kw["keep"] = keep

    def walk(call):
        codes = torch.full((B, img), -1, dtype=torch.int64, device=cuda)
        tok = torch.zeros(B, dtype=torch.int64, device=cuda)
        toks = []
        for pos in range(T + img - 1):
            call(logits[pos], _i32(pos, cuda), text, codes, tok, vt, **kw)
            toks.append(tok.clone())
        return codes, torch.stack(toks)

    codes, toks = walk(lambda lg, p, *rest, **k: C.sample_step(lg, 0, 1.0, 1.0, _i64(0, cuda), p, *rest, **k,
                                                               **_tables(MIXED, MIXED_SEEDS, cuda)))
    for r, ((k_, tp, t), s) in enumerate(zip(MIXED, MIXED_SEEDS)):
        wc, wt = walk(lambda lg, p, *rest, **k: C.sample_step(lg, k_, tp, t, _i64(s, cuda), p, *rest, **k))
        assert torch.equal(codes[r], wc[r]) and torch.equal(toks[:, r], wt[:, r]), (mode, r)
    if mode != "plain":
        assert torch.equal(codes[:, :3], prime[:, :3])
    if mode == "keep":
        assert torch.equal(codes[keep.bool()], prime[keep.bool()])


@pytest.mark.parametrize("V", [8192, 1000])
@pytest.mark.parametrize("b", [1, 4])
def test_guided_rows(cuda, b, V):
    T, img, vt, C = 6, 9, 1000, _C()
    g = torch.Generator().manual_seed(b * V)
    logits = (torch.randn(2 * b, V, generator=g) * 2).to(cuda)
    text = torch.randint(2, 900, (2 * b, T), generator=g).to(cuda)
    scales_all = [0.0, 1.0, 3.0, 7.5]
    one = _f32([1.0], cuda)
    for scales in ([scales_all] if b == 4 else [[s] for s in scales_all]):
        params, seeds = [MIXED[(r + 1) % 4] for r in range(b)], MIXED_SEEDS[:b]
        for pos in (2, 7):  # the caption, then an image position
            codes = torch.full((2 * b, img), -1, dtype=torch.int64, device=cuda)
            tok = torch.full((2 * b,), -1, dtype=torch.int64, device=cuda)
            got = C.sample_step(logits, 0, 1.0, 1.0, _i64(0, cuda), _i32(pos, cuda), text, codes, tok, vt, cond_scale=one,
                                row_cond_scale=_f32(scales, cuda), **_tables(params, seeds, cuda))
            assert got.shape == (b,)
            for r in range(b):
                wcodes, wtok = torch.full_like(codes, -1), torch.full_like(tok, -1)
                k_, tp, t = params[r]
                want = C.sample_step(logits, k_, tp, t, _i64(seeds[r], cuda), _i32(pos, cuda), text, wcodes, wtok, vt,
                                     cond_scale=_f32([scales[r]], cuda))
                assert got[r].item() == want[r].item(), (b, V, pos, r)
                for rr in (r, r + b):  # both halves' codes and tokens
                    assert torch.equal(codes[rr], wcodes[rr]) and tok[rr].item() == wtok[rr].item()
            assert (tok >= 0).all()


def test_rejections(cuda):
    C, V = _C(), 64
    logits = torch.randn(B, V, device=cuda)
    pos, sd = _i32(0, cuda), _i64(0, cuda)
    good = _tables(MIXED, MIXED_SEEDS, cuda)

    def bad(**kw):
        with pytest.raises(RuntimeError, match="sample:"):
            C.sample_step(logits, 0, 1.0, 1.0, sd, pos, **kw)

    C.sample_step(logits, 0, 1.0, 1.0, sd, pos, **good)
    for name in good:  # three of the four
        bad(**{k: v for k, v in good.items() if k != name})
    bad(noise_row=_i32([0, 1, 2, 3], cuda))  # noise_row alone
    wrong = {"row_top_k": torch.int64, "row_top_p": torch.float64, "row_temperature": torch.float16, "row_seed": torch.int32}
    for name, dt in wrong.items():
        bad(**{**good, name: good[name].to(dt)})
    bad(**good, noise_row=torch.arange(B, device=cuda))  # int64
    for name in good:
        bad(**{**good, name: good[name][:3].contiguous()})  # wrong length
        bad(**{**good, name: good[name].view(B, 1)})  # 2-D
        bad(**{**good, name: good[name].cpu()})
        bad(**{**good, name: good[name].repeat_interleave(2)[::2]})  # not contiguous
    bad(**good, noise_row=_i32([0, 1, 2], cuda))
    bad(**good, row_cond_scale=_f32([1.0] * B, cuda))  # row_cond_scale without cond_scale
    one = _f32([1.0], cuda)
    half = _tables(MIXED[:2], MIXED_SEEDS[:2], cuda)
    C.sample_step(logits, 0, 1.0, 1.0, sd, pos, cond_scale=one, row_cond_scale=_f32([1.0, 2.0], cuda), **half)
    bad(cond_scale=one, **half)  # guided tables without row_cond_scale
    bad(cond_scale=one, row_cond_scale=_f32([1.0] * B, cuda), **good)  # guided tables of length 2 b
    bad(cond_scale=one, row_cond_scale=_f32([1.0] * B, cuda), **half)
    bad(cond_scale=one, row_cond_scale=_f32([1.0, 2.0], cuda).double(), **half)


# -- engines --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["plain_stack", "reversible"])
def setup(request, cuda):
    torch.manual_seed(0)
    cfg = tiny(request.param)
    m = DALLE(cfg).eval().to(cuda)
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len), device=cuda)
    image = torch.randint(0, cfg.num_image_tokens, (B, cfg.image_seq_len), generator=torch.Generator().manual_seed(3)).to(cuda)
    regen = torch.zeros(B, cfg.image_seq_len, dtype=torch.bool, device=cuda)
    regen[0, 19:] = True
    regen[1, 7] = True
    regen[2] = True
    regen[3, 40:90] = True
    return cfg, m, m.prepare_text(text), image, regen


def _forms(image, regen):
    return {"plain": {}, "prime": {"prime": image[:, :19]}, "inpaint": {"image": image, "regen": regen}}


@pytest.mark.parametrize("use_graph", [True, False])
def test_contract_1_uniform_tables_equal_the_plain_engine(cuda, setup, use_graph):
    cfg, m, tb, image, regen = setup
    plain, rows = DecodeEngine(m, B, device=cuda), DecodeEngine(m, B, device=cuda, row_params=True)
    assert rows.fused_sampler
    for name, kw in _forms(image, regen).items():
        want = plain.generate(tb, temperature=0.9, top_k=16, top_p=0.95, seed=5, use_graph=use_graph, **kw)
        got = rows.generate(tb, temperature=[0.9] * B, top_k=[16] * B, top_p=[0.95] * B, seed=[5] * B, use_graph=use_graph, **kw)
        assert torch.equal(got, want), name
        assert torch.equal(rows.generate(tb, temperature=0.9, top_k=16, top_p=0.95, seed=5, use_graph=use_graph, **kw), want)


def test_contract_2_split_engine(cuda, setup):
    cfg, m, tb, image, regen = setup
    plain = SplitDecodeEngine(m, B, device=cuda, parts=2)
    rows = SplitDecodeEngine(m, B, device=cuda, parts=2, row_params=True)
    b, s = B // 2, 5
    seeds, noise = [s + j // b for j in range(B)], [j % b for j in range(B)]
    for name, kw in _forms(image, regen).items():
        want = plain.generate(tb, top_k=16, seed=s, **kw)
        got = rows.generate(tb, top_k=16, seed=seeds, noise_row=noise, **kw)
        assert torch.equal(got, want), name
    eager = rows.generate(tb, top_k=16, seed=seeds, noise_row=noise, use_graph=False)
    assert torch.equal(eager, plain.generate(tb, top_k=16, seed=s))


def _mixed_kw():
    return {"temperature": [p[2] for p in MIXED], "top_k": [p[0] for p in MIXED], "top_p": [p[1] for p in MIXED],
            "seed": list(MIXED_SEEDS)}


def test_contract_3_mixed_rows(cuda, setup):
    cfg, m, tb, image, regen = setup
    plain, rows = DecodeEngine(m, B, device=cuda), DecodeEngine(m, B, device=cuda, row_params=True)
    got = rows.generate(tb, **_mixed_kw())
    for j, ((k, tp, t), s) in enumerate(zip(MIXED, MIXED_SEEDS)):
        want = plain.generate(tb, temperature=t, top_k=k, top_p=tp, seed=s)
        assert torch.equal(got[j], want[j]), j
    assert len({tuple(r) for r in got.tolist()}) == B


def test_contract_3_mixed_rows_split(cuda, setup):
    """The plain split engine keys part ``i``'s noise by (seed + i, row within the part), so the mixed call that its
    four scalar calls reproduce takes ``noise_row[j] = j % b`` and is compared with the scalar call of seed
    ``s_j - j // b``. With ``noise_row = j`` (the default) row ``j`` is instead the row engine's own uniform call."""
    cfg, m, tb, image, regen = setup
    plain = SplitDecodeEngine(m, B, device=cuda, parts=2)
    rows = SplitDecodeEngine(m, B, device=cuda, parts=2, row_params=True)
    b = B // 2
    got = rows.generate(tb, noise_row=[j % b for j in range(B)], **_mixed_kw())
    default = rows.generate(tb, **_mixed_kw())
    for j, ((k, tp, t), s) in enumerate(zip(MIXED, MIXED_SEEDS)):
        want = plain.generate(tb, temperature=t, top_k=k, top_p=tp, seed=s - j // b)
        assert torch.equal(got[j], want[j]), j
        uniform = rows.generate(tb, temperature=t, top_k=k, top_p=tp, seed=s)
        assert torch.equal(default[j], uniform[j]), j


def test_contract_3_guided(cuda, setup):
    cfg, m, tb, image, regen = setup
    plain = DecodeEngine(m, B, device=cuda, guided=True)
    rows = DecodeEngine(m, B, device=cuda, guided=True, row_params=True)
    scales = [3.0, 0.5, 3.0, 0.5]
    got = rows.generate(tb, cond_scale=scales, **_mixed_kw())
    assert torch.equal(rows.codes[:B], rows.codes[B:])
    for j, ((k, tp, t), s) in enumerate(zip(MIXED, MIXED_SEEDS)):
        want = plain.generate(tb, temperature=t, top_k=k, top_p=tp, seed=s, cond_scale=scales[j])
        assert torch.equal(got[j], want[j]), j


@pytest.mark.parametrize("split", [False, True])
def test_contract_4_one_graph(cuda, setup, split, monkeypatch):
    cfg, m, tb, image, regen = setup
    eng = (SplitDecodeEngine(m, B, device=cuda, parts=2, row_params=True) if split
           else DecodeEngine(m, B, device=cuda, row_params=True))
    first = eng.generate(tb, **_mixed_kw())
    graph = eng.graph
    part_graphs = [p.graph for p in eng.parts] if split else None
    assert graph is not None
    steps = []
    for p in (eng.parts if split else [eng]):  # a warm-up or an eager step would come through here
        monkeypatch.setattr(p, "_step_rows", lambda *a, **k: steps.append(1))
    other = eng.generate(tb, temperature=0.5, top_k=[4, 0, 0, 64], top_p=0.9, seed=[1, 2, 3, 4], noise_row=[9, 8, 7, 6])
    assert eng.graph is graph and not torch.equal(other, first)
    again = eng.generate(tb, **_mixed_kw())
    assert eng.graph is graph and torch.equal(again, first) and not steps
    if split:
        assert [p.graph for p in eng.parts] == part_graphs


def test_plain_engine_names_the_flag(cuda, setup):
    cfg, m, tb, image, regen = setup
    for eng in (DecodeEngine(m, B, device=cuda), SplitDecodeEngine(m, B, device=cuda, parts=2)):
        with pytest.raises(ValueError, match="row_params=True"):
            eng.generate(tb, top_k=[1, 2, 3, 4])
        with pytest.raises(ValueError, match="row_params=True"):
            eng.generate(tb, noise_row=[0, 1, 2, 3])


def test_generate_images_seed_replays(cuda, setup):
    cfg, m, tb, image, regen = setup
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len), device=cuda)
    a = m.generate_images(text, seed=11, top_k=16)
    assert torch.equal(m.generate_images(text, seed=11, top_k=16), a)  # the plain engine, its seed now reachable
    assert not torch.equal(m.generate_images(text, seed=12, top_k=16), a)
    plain = m._decode_engine
    assert not plain.row_params
    rows = m.generate_images(text, seed=[11] * B, top_k=16)
    assert m._decode_engine is plain and m._row_decode_engine.row_params
    if type(plain).__name__ == "DecodeEngine":  # contract 1 through the public call
        assert torch.equal(rows, a)


def test_serving_mixed_requests(cuda):
    """``mix_params``: an unguided and a guided pair of requests, each pair with two parameter sets, each in one batch."""
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
    # two pictures fill a batch: a pair runs as soon as its second request arrives
    gen = BatchingGenerator(model, HashingTokenizer(vocab_size=cfg.num_text_tokens), cuda, max_batch=2, batch_window_ms=60000,
                            mix_params=True)
    try:
        futs = [gen.submit(["a red apple"], temperature=1.0, top_k=32, seed=7), gen.submit(["a cat"], temperature=0.0, top_p=0.9),
                gen.submit(["a dog"], top_k=16, cond_scale=3.0), gen.submit(["a bird"], temperature=0.7, cond_scale=0.5, seed=9)]
        res = [f.result(timeout=100) for f in futs]
        assert all(r["batch_images"] == 2 and r["batch_padded"] == 2 and len(r["codes"]) == 1 for r in res)
        assert sorted(gen.row_engines) == [2] and sorted(gen.guided_row_engines) == [2]
        assert not gen.engines and not gen.guided_engines
        eng, geng = gen.row_engines[2], gen.guided_row_engines[2]
        assert eng.row_params and not eng.guided and geng.row_params and geng.guided
        assert geng.row_cond_scale.tolist() == [3.0, 0.5] and eng.row_top_k.tolist() == [32, 0]
        assert res[0]["seed"] == 7 and res[3]["seed"] == 9 and isinstance(res[1]["seed"], int)
        graph = eng.graph
        assert graph is not None
        again = [gen.submit(["a red apple"], temperature=1.0, top_k=32, seed=7), gen.submit(["a fish"], top_p=0.5)]
        assert again[0].result(timeout=100)["codes"] == res[0]["codes"] and again[1].result(timeout=100)["batch_images"] == 2
        assert gen.row_engines[2] is eng and eng.graph is graph
    finally:
        gen.close()
