"""Inpainting on MI355X: the fused sampler's ``keep`` table, the prefill kernels' image geometry and query-block
softmax (``csrc/kernels/sample.hip``, ``decode.hip``) and the decode engines that use them (eager, hipGraph replay,
split and guided engines; ``models/generation.py``)."""
import copy

import pytest
import torch

from dalle_amd.config import DALLEConfig, tiny
from dalle_amd.models.dalle import DALLE
from dalle_amd.models.generation import DecodeEngine, SplitDecodeEngine

pytestmark = pytest.mark.gpu

B = 4


def _cfg():
    c = tiny(False)
    return DALLEConfig(**{**c.to_dict(), "depth": 4, "attn_types": ["axial_row", "axial_col", "conv_like", "full"],
                          "shared_attn_ids": [0, 1, 2, 3], "shared_ff_ids": [0, 1, 0, 1]})


def _C():
    from dalle_amd.ops.hip_ops import C

    return C()


def suffix_mask(k, dev, L=256):
    return (torch.arange(L, device=dev) >= k).expand(B, L).clone()


def rect_mask(dev, S=16):
    m = torch.zeros(B, S, S, dtype=torch.bool, device=dev)
    m[:, 5:10, 3:12] = True  # grid rows 5..9 x cols 3..11: k0 = 83, last = 155
    return m.reshape(B, S * S)


def per_row_mask(dev, L=256):
    m = torch.zeros(B, L, dtype=torch.bool, device=dev)
    m[0, 19:] = True
    m[1, 0] = True
    m[2] = True
    m[3, 255] = True
    return m


@pytest.fixture(scope="module")
def setup(cuda):
    torch.manual_seed(0)
    cfg = _cfg()
    m = DALLE(cfg).eval().to(cuda)
    text = torch.randint(2, cfg.num_text_tokens, (B, cfg.text_seq_len), device=cuda)
    tb = m.prepare_text(text)
    image = torch.randint(0, cfg.num_image_tokens, (B, cfg.image_seq_len), generator=torch.Generator().manual_seed(3)).to(cuda)
    return cfg, m, tb, image


# -- kernels alone ------------------------------------------------------------------------------------------------
def test_sample_step_keep(cuda):
    Bs, T, img, vt, V = 4, 6, 9, 1000, 64
    g = torch.Generator().manual_seed(0)
    text = torch.randint(2, 900, (Bs, T), generator=g).to(cuda)
    logits = torch.randn(Bs, V, generator=g).to(cuda)
    prime = torch.randint(0, V, (Bs, img), generator=g).to(cuda)
    seed = torch.tensor(5, dtype=torch.int64, device=cuda)
    keep = torch.zeros(Bs, img, dtype=torch.bool)
    keep[0, :3] = True
    keep[1, 4] = True
    keep[3, 0] = keep[3, 8] = True  # row 2 keeps nothing
    keep = keep.to(cuda)
    C = _C()

    def run(n_prime=None, keep=None):
        codes = torch.full((Bs, img), -1, dtype=torch.int64, device=cuda)
        tok = torch.zeros(Bs, dtype=torch.int64, device=cuda)
        toks, raw = [], []
        kw = {}
        if n_prime is not None:
            kw = dict(prime=prime, n_prime=torch.tensor(n_prime, dtype=torch.int32, device=cuda))
        if keep is not None:
            kw["keep"] = keep
        for pos in range(T + img - 1):
            p = torch.tensor(pos, dtype=torch.int32, device=cuda)
            raw.append(C.sample_step(logits, 0, 1.0, 1.0, seed, p, text, codes, tok, vt, **kw).clone())
            toks.append(tok.clone())
        return codes, torch.stack(toks), torch.stack(raw)  # toks / raw: (position, row)

    base_codes, base_tok, base_raw = run()
    for kp in (keep, keep.to(torch.uint8)):
        codes, toks, raw = run(0, kp)
        assert torch.equal(codes, torch.where(keep, prime, base_codes))
        assert torch.equal(toks[:T - 1], base_tok[:T - 1])  # the caption positions
        kt = keep.t()  # (image position, row)
        assert torch.equal(toks[T - 1:], torch.where(kt, prime.t() + vt, base_tok[T - 1:]))
        assert torch.equal(raw[T - 1:], torch.where(kt, prime.t(), base_raw[T - 1:]))
        assert torch.equal(raw[:T - 1], base_raw[:T - 1])
    # a zero mask is no mask
    c0, t0, r0 = run(0, torch.zeros_like(keep))
    assert torch.equal(c0, base_codes) and torch.equal(t0, base_tok) and torch.equal(r0, base_raw)
    # keep ORs with n_prime
    codes, toks, raw = run(2, keep)
    forced = keep | (torch.arange(img, device=cuda) < 2)
    assert torch.equal(codes, torch.where(forced, prime, base_codes))
    assert torch.equal(raw[T - 1:], torch.where(forced.t(), prime.t(), base_raw[T - 1:]))

    # the argument checks, before any launch
    def call(**kw):
        a = dict(prime=prime, n_prime=torch.tensor(0, dtype=torch.int32, device=cuda), keep=keep)
        a.update(kw)
        a = {k: v for k, v in a.items() if v is not None}
        C.sample_step(logits, 0, 1.0, 1.0, seed, torch.tensor(0, dtype=torch.int32, device=cuda), text,
                      torch.zeros(Bs, img, dtype=torch.int64, device=cuda), torch.zeros(Bs, dtype=torch.int64, device=cuda),
                      vt, **a)

    call()
    for bad in (dict(prime=None, n_prime=None), dict(keep=keep[:, :5].contiguous()), dict(keep=keep[:2].contiguous()),
                dict(keep=keep.long()), dict(keep=keep.cpu()), dict(keep=keep.t().contiguous().t())):
        with pytest.raises(RuntimeError, match="keep"):
            call(**bad)


def test_sample_step_keep_guided(cuda):
    """Guided form: the table is indexed by the picture row r < b, and both rows r / r + b take the code."""
    b, T, img, vt, V = 2, 6, 9, 1000, 64
    g = torch.Generator().manual_seed(1)
    text = torch.randint(2, 900, (2 * b, T), generator=g).to(cuda)
    logits = torch.randn(2 * b, V, generator=g).to(cuda)
    prime = torch.randint(0, V, (2 * b, img), generator=g).to(cuda)
    seed = torch.tensor(7, dtype=torch.int64, device=cuda)
    scale = torch.full((1,), 1.5, device=cuda)
    keep = torch.zeros(b, img, dtype=torch.bool, device=cuda)
    keep[0, 1] = keep[1, 5] = keep[1, 6] = True
    C = _C()

    def run(keep=None):
        codes = torch.full((2 * b, img), -1, dtype=torch.int64, device=cuda)
        tok = torch.zeros(2 * b, dtype=torch.int64, device=cuda)
        toks = []
        kw = dict(prime=prime, n_prime=torch.tensor(0, dtype=torch.int32, device=cuda), cond_scale=scale)
        if keep is not None:
            kw["keep"] = keep
        for pos in range(T + img - 1):
            C.sample_step(logits, 16, 1.0, 1.0, seed, torch.tensor(pos, dtype=torch.int32, device=cuda), text, codes, tok, vt, **kw)
            toks.append(tok.clone())
        return codes, torch.stack(toks)

    base_codes, base_tok = run()
    codes, toks = run(keep)
    want = torch.where(keep, prime[:b], base_codes[:b])
    assert torch.equal(codes[:b], want) and torch.equal(codes[b:], want)
    want_tok = torch.where(keep.t(), prime[:b].t() + vt, base_tok[T - 1:, :b])
    assert torch.equal(toks[T - 1:, :b], want_tok) and torch.equal(toks[T - 1:, b:], want_tok)
    with pytest.raises(RuntimeError, match="keep"):  # one row per picture, not per logits row
        run(torch.zeros(2 * b, img, dtype=torch.bool, device=cuda))


@pytest.mark.parametrize("D", [256, 1024])
def test_prefill_ln_shift_with_image_rows(cuda, D):
    """LN + shift over the caption and k image positions (T 5, S 4): every shifted channel of ``out`` is bitwise the
    history element the decode rule names -- the cell above for channels [0, D/4), the cell to the left for
    [D/4, D/2), the previous position in the caption -- or zero where it names none."""
    Bn, T, S, n = 2, 5, 4, 21
    torch.manual_seed(0)
    w, b = torch.randn(D, device=cuda), torch.randn(D, device=cuda)
    q, h2 = D // 4, D // 2
    for k in (0, 1, 4, 5, 11):
        P = T - 1 + k
        x = torch.randn(Bn, P, D, device=cuda) * 2 + 0.5
        hist = torch.zeros(Bn, n, D, dtype=torch.bfloat16, device=cuda)
        out = torch.full((Bn, P, D), 7.0, dtype=torch.bfloat16, device=cuda)
        _C().prefill_ln_shift_(x, w, b, hist, out, True, 1e-5, T, S)
        y = torch.nn.functional.layer_norm(x, (D,), w, b, 1e-5)
        assert (hist[:, :P].float() - y).abs().max().item() < 0.05
        assert torch.count_nonzero(hist[:, P:]) == 0
        zero = torch.zeros(Bn, D, dtype=torch.bfloat16, device=cuda)
        for p in range(P):
            if p < T:
                up = left = hist[:, p - 1] if p >= 1 else zero
            else:
                ki = p - T
                up = hist[:, p - S] if ki >= S else zero
                left = hist[:, p - 1] if ki % S else zero
            assert torch.equal(out[:, p, :q], up[:, :q]), (k, p)
            assert torch.equal(out[:, p, q:h2], left[:, q:h2]), (k, p)
            assert torch.equal(out[:, p, h2:], hist[:, p, h2:]), (k, p)
        # no shift: the LN output everywhere; the default geometry: every row is a caption row (the existing call)
        out2 = torch.empty_like(out)
        _C().prefill_ln_shift_(x, w, b, torch.zeros_like(hist), out2, False, 1e-5, T, S)
        assert torch.equal(out2, hist[:, :P])
        out3, out4 = torch.empty_like(out), torch.empty_like(out)
        _C().prefill_ln_shift_(x, w, b, torch.zeros_like(hist), out3, True, 1e-5)
        _C().prefill_ln_shift_(x, w, b, torch.zeros_like(hist), out4, True, 1e-5, P, S)
        assert torch.equal(out3, out4)
        assert torch.equal(out3[:, 1:, :h2], hist[:, :P - 1, :h2]) and torch.count_nonzero(out3[:, 0, :h2]) == 0


@pytest.mark.parametrize("Pk", [513, 700, 1279])
def test_prefill_softmax_block(cuda, Pk):
    R = 2
    torch.manual_seed(Pk)
    mask = torch.tril(torch.ones(Pk + 3, Pk + 5, dtype=torch.bool, device=cuda))  # wider than the keys: a row stride of its own
    mask[300, :3] = False  # a non-causal hole
    mask[5, 2] = False
    for q0, Q in ((0, Pk), (256, 100)):
        sc = torch.randn(R, Q, Pk, device=cuda) * 3
        pr = torch.full((R, Q, Pk), 9.0, dtype=torch.bfloat16, device=cuda)
        _C().prefill_softmax_block_(sc, mask, pr, q0)
        mq = mask[q0:q0 + Q, :Pk]
        ref = torch.softmax(sc.masked_fill(~mq, float("-inf")), -1)
        assert (pr.float() - ref).abs().max().item() < 4e-3
        assert torch.count_nonzero(pr.float() * (~mq).float()) == 0
    with pytest.raises(RuntimeError, match="mask"):
        _C().prefill_softmax_block_(sc, mask, pr, Pk)  # queries past the mask's rows
    with pytest.raises(RuntimeError, match="2048"):
        big = torch.zeros(1, 1, 2049, device=cuda)
        _C().prefill_softmax_block_(big, torch.ones(4, 2049, dtype=torch.bool, device=cuda), big.to(torch.bfloat16), 0)


# -- engines ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_stepwise_mask_equals_prefix(cuda, setup, use_graph):
    """A suffix mask with the kept head fed step by step is the ``prime=`` call, bit for bit."""
    cfg, m, tb, image = setup
    k = 19
    eng = DecodeEngine(m, B, device=cuda)
    assert eng.fused_sampler
    a = eng.generate(tb, top_k=16, seed=5, use_graph=use_graph, image=image, regen=suffix_mask(k, cuda), prefill_kept=False)
    b = eng.generate(tb, top_k=16, seed=5, use_graph=use_graph, prime=image[:, :k])
    assert torch.equal(a, b) and torch.equal(a[:, :k], image[:, :k])


def test_graph_replay_equals_eager_and_skip_tail(cuda, setup):
    cfg, m, tb, image = setup
    regen = rect_mask(cuda)
    eng = DecodeEngine(m, B, device=cuda)
    eager = eng.generate(tb, top_k=16, seed=5, use_graph=False, image=image, regen=regen)
    graph = eng.generate(tb, top_k=16, seed=5, use_graph=True, image=image, regen=regen)
    assert torch.equal(eager[~regen], image[~regen])
    assert torch.equal(eager, graph)
    full_tail = eng.generate(tb, top_k=16, seed=5, use_graph=True, image=image, regen=regen, skip_tail=False)
    assert torch.equal(full_tail, graph)
    # all kept: the input, nothing runs; all True: the unprimed call
    assert torch.equal(eng.generate(tb, top_k=16, seed=5, image=image, regen=torch.zeros_like(regen)), image)
    assert torch.equal(eng.generate(tb, top_k=16, seed=5, image=image, regen=torch.ones_like(regen)),
                       eng.generate(tb, top_k=16, seed=5))


def test_one_graph_serves_every_mode(cuda, setup):
    cfg, m, tb, image = setup
    fresh = DecodeEngine(m, B, device=cuda).generate(tb, top_k=16, seed=5, use_graph=True)
    eng = DecodeEngine(m, B, device=cuda)
    a = eng.generate(tb, top_k=16, seed=5, use_graph=True)
    graph = eng.graph
    assert graph is not None and torch.equal(a, fresh)
    regen = per_row_mask(cuda)
    b = eng.generate(tb, top_k=16, seed=5, use_graph=True, image=image, regen=regen)
    assert eng.graph is graph and torch.equal(b[~regen], image[~regen])
    assert torch.equal(b[2], fresh[2])  # the all-True row of the set: an ordinary row (same noise, same rows)
    c = eng.generate(tb, top_k=16, seed=6, use_graph=True, prime=image[:, :19])
    assert eng.graph is graph and torch.equal(c[:, :19], image[:, :19])
    d = eng.generate(tb, top_k=16, seed=5, use_graph=True)
    assert eng.graph is graph and torch.equal(d, fresh)
    assert not eng.keep.any() and int(eng.n_prime) == 0


def test_unfused_step_applies_the_same_rule(cuda, setup):
    cfg, m, tb, image = setup
    regen = per_row_mask(cuda)
    fused = DecodeEngine(m, B, device=cuda).generate(tb, top_k=1, seed=5, use_graph=False, image=image, regen=regen)
    plain = DecodeEngine(m, B, device=cuda, fused_sampler=False).generate(tb, top_k=1, seed=5, use_graph=False, image=image,
                                                                         regen=regen)
    assert torch.equal(plain[~regen], image[~regen])
    assert (plain == fused).float().mean().item() > 0.98


def test_split_engine(cuda, setup):
    cfg, m, tb, image = setup
    regen = per_row_mask(cuda)
    regen[:, :5] = False  # a global k0 of 5 (row 2's), per-row masks behind it: rows 0 / 1 and 2 / 3 go to different parts
    single = DecodeEngine(m, B, device=cuda).generate(tb, top_k=1, seed=5, image=image, regen=regen)
    split = SplitDecodeEngine(m, B, device=cuda, parts=2)
    got = split.generate(tb, top_k=1, seed=5, image=image, regen=regen)
    assert torch.equal(got[~regen], image[~regen])
    assert (got == single).float().mean().item() > 0.98
    eager = split.generate(tb, top_k=1, seed=5, image=image, regen=regen, use_graph=False)
    assert torch.equal(eager, got)
    with pytest.raises(ValueError, match="image"):
        split.generate(tb, top_k=1, seed=5, image=image[:2], regen=regen)


def test_guided_engine(cuda, setup):
    cfg, m, tb, image = setup
    regen = rect_mask(cuda)
    eng = DecodeEngine(m, B, device=cuda, guided=True)
    out = eng.generate(tb, top_k=16, seed=5, image=image, regen=regen, cond_scale=2.0)
    assert torch.equal(out[~regen], image[~regen])
    assert torch.equal(eng.codes[:B], eng.codes[B:])
    stepwise = eng.generate(tb, top_k=16, seed=5, image=image, regen=regen, cond_scale=2.0, prefill_kept=False,
                            skip_tail=False)
    assert torch.equal(stepwise[~regen], image[~regen])
    assert (out == stepwise).float().mean().item() > 0.9  # another summation order ahead of position 83
    with pytest.raises(ValueError, match="image"):
        eng.generate(tb, image=image[:2], regen=regen[:2], cond_scale=2.0)


@pytest.fixture(scope="module")
def teacher(setup):
    """fp32 logits of the CPU engine, teacher-forced on the picture, same weights."""
    cfg, m, tb, image = setup
    cpu = copy.deepcopy(m).float().cpu()
    with torch.no_grad():
        return DecodeEngine(cpu, B, device=torch.device("cpu"), use_hip=False).teacher_forced_logits(tb.cpu(), image.cpu())


@pytest.mark.parametrize("k0", [17, 83])
def test_kept_head_numerics(cuda, setup, teacher, k0):
    """The logits of the first regenerated position after (a) the batched pass over the kept head, (b) the same codes
    fed as decode steps, each against the fp32 CPU engine. Both are bf16 paths that differ in summation order and GEMM
    routing only, so (a) may be at most 2 x as far off as (b) -- (b)'s error is measured here, not fixed in advance.
    (c): (a) with the scores in several query blocks, as a pass longer than 512 positions runs. Measured on MI355X:
    see profiles/inpaint_numerics.txt."""
    cfg, m, tb, image = setup
    ref = teacher[:, k0].to(cuda)

    def stepwise(eng):
        eng.prefill_parallel(tb)
        for i in range(k0):
            eng._forward_position()
            eng.tok.copy_(image[:, i] + eng.Vt)
            eng.pos.add_(1)
        return eng._forward_position().float()

    def batched(eng):
        eng.prefill_parallel(tb, kept=image[:, :k0])
        assert int(eng.pos) == cfg.text_len - 1 + k0 and torch.equal(eng.tok, image[:, k0 - 1] + eng.Vt)
        return eng._forward_position().float()

    with torch.no_grad():
        err_b = (stepwise(DecodeEngine(m, B, device=cuda)) - ref).abs().max().item()
        err_a = (batched(DecodeEngine(m, B, device=cuda)) - ref).abs().max().item()
        blocked = DecodeEngine(m, B, device=cuda)
        blocked.pf_dense_max, blocked.pf_query_block = 64, 48
        err_c = (batched(blocked) - ref).abs().max().item()
    print(f"\nkept-head numerics k0={k0}: max |logit - fp32| batched {err_a:.5f}, blocked {err_c:.5f}, stepwise {err_b:.5f}, "
          f"logits max |.| {ref.abs().max().item():.3f}")
    assert err_a <= 2 * err_b, (err_a, err_b)
    assert err_c <= 2 * err_b, (err_c, err_b)
