"""Pins ``tests/attn_ref.py`` -- the float64 reference and the seeded inputs of ``test_attention_kernels_gpu.py`` --
without a GPU: the reference against ``ops.reference`` + float64 autograd, the mask against a brute force written from
``models/patterns.py``'s docstring, the storage helpers, and two conditions on the inputs themselves: every planted
probe is sensitive (admitting its one forbidden key moves the reference by >= 100 x the bound the GPU test asserts),
and the ramp data crosses the forward's rescale threshold in the fast heads and never in the slow ones."""
import math

import pytest
import torch

import attn_ref as ar
from dalle_amd.models.patterns import AttnGeometry, allowed, storage_index
from dalle_amd.ops import reference as ref

PATTERNS = ["full", "axial_row", "axial_col", "conv_like"]


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("T,S", [(1, 8), (5, 8), (33, 8), (32, 16), (40, 16)])
@pytest.mark.parametrize("attn_type,K", [("full", 5), ("axial_row", 5), ("axial_col", 5), ("conv_like", 1), ("conv_like", 3),
                                         ("conv_like", 5), ("conv_like", 9)])
def test_reference_matches_torch_autograd(attn_type, T, S, K):
    """Forward, lse, dQ / dK / dV and the rotary-folded dqkv against ops.reference in float64 + autograd, 1e-12."""
    case = ar.Case(T, S, attn_type, K, B=2, H=2)
    g = torch.Generator().manual_seed(T * 100 + S + K)
    qkv = torch.randn(case.B, case.n, 3 * case.H * 64, generator=g, dtype=torch.float64).requires_grad_(True)
    dout = torch.randn(case.B, case.n, case.H * 64, generator=g, dtype=torch.float64)
    cos, sin = ar.tables64(case)
    q, k, v = ref.qkv_rotary(qkv, case.H, cos, sin)
    q.retain_grad(), k.retain_grad(), v.retain_grad()
    out = ref.sparse_attention_core(q, k, v, case.geom, attn_type)
    out.backward(dout)
    i = torch.arange(case.n)
    mask = allowed(case.geom, attn_type, i.view(-1, 1), i.view(1, -1))
    lse_t = torch.logsumexp((q @ k.transpose(-1, -2)).masked_fill(~mask, -math.inf), dim=-1).detach() * ar.LOG2E

    qs, ks, vs = ar.rope_fwd_ref(qkv.detach(), case)
    for got, want in zip((qs, ks, vs), (q, k, v)):
        assert _rel(ar.unpack(got, case), want.detach()) < 1e-12
    dOs = ar.pack(ar.tokens_to_heads(dout, case.H), case)
    r = ar.attention_ref(qs, ks, vs, case, dO=dOs)
    assert _rel(ar.heads_to_tokens(ar.unpack(r["O"], case)), out.detach()) < 1e-12
    assert _rel(ar.unpack(r["lse"], case), lse_t) < 1e-12
    for name, t in (("dQ", q), ("dK", k), ("dV", v)):
        assert _rel(ar.unpack(r[name], case), t.grad) < 1e-12, name
    assert _rel(ar.rope_bwd_ref(r["dQ"], r["dK"], r["dV"], case), qkv.grad) < 1e-12
    # rows without a sequence position: no probability, no gradient
    pad = ~r["real"]
    assert r["P"][:, pad].abs().max() == 0 and r["P"][:, :, pad].abs().max() == 0
    assert r["dK"][:, pad].abs().max() == 0 and r["dV"][:, pad].abs().max() == 0


def _brute_force_allowed(T, S, K, attn_type, i, j):
    """From the module docstring of models/patterns.py, one (query, key) pair at a time."""
    if j > i:
        return False
    if j < T:
        return True          # text keys: causal for text queries (j <= i), all of them for image queries
    if i < T:
        return False
    qr, qc = divmod(i - T, S)
    kr, kc = divmod(j - T, S)
    if attn_type == "full":
        return True
    if attn_type == "axial_row":
        return qr == kr and kc <= qc
    if attn_type == "axial_col":
        return qc == kc and kr <= qr
    return qr - K + 1 <= kr <= qr and qc - K + 1 <= kc <= qc


@pytest.mark.parametrize("T,S,K", [(3, 8, 1), (3, 8, 3), (5, 8, 9), (4, 16, 5), (33, 16, 3)])
@pytest.mark.parametrize("attn_type", PATTERNS)
def test_allowed_matches_brute_force(attn_type, T, S, K):
    geom = AttnGeometry(T, S, K)
    n = geom.seq_len
    i = torch.arange(n)
    got = allowed(geom, attn_type, i.view(-1, 1), i.view(1, -1))
    want = torch.zeros(n, n, dtype=torch.bool)
    for a in range(n):
        for b in range(n):
            want[a, b] = _brute_force_allowed(T, S, K, attn_type, a, b)
    assert torch.equal(got, want)


@pytest.mark.parametrize("attn_type", ["axial_row", "axial_col"])
@pytest.mark.parametrize("T,S", [(1, 8), (33, 16), (40, 64)])
def test_storage_round_trip(attn_type, T, S):
    case = ar.Case(T, S, attn_type, 5, B=2, H=3)
    x = torch.arange(case.BH * case.n * 64, dtype=torch.float64).reshape(case.B, case.H, case.n, 64) + 1.0
    xs = ar.pack(x, case, fill=-7.0)
    assert xs.shape == (case.BH, case.Np, 64)
    assert torch.equal(ar.unpack(xs, case), x)
    s2q = ar.storage_to_seq(case)
    assert (s2q >= 0).sum() == case.n and (xs[:, s2q < 0] == -7.0).all()
    assert (s2q[case.T:case.Tp] == -1).all() and torch.equal(s2q[:T], torch.arange(T))
    # image token (r, c) sits at Tp + r S + c, column-major (Tp + c S + r) for axial_col
    for r, c in [(0, 0), (0, S - 1), (S - 1, 0), (3, 5), (S - 2, S - 1)]:
        row = case.Tp + (c * S + r if attn_type == "axial_col" else r * S + c)
        assert int(s2q[row]) == T + r * S + c
    assert int(s2q[case.Np - 1]) == -1   # the dropped last image token, last row in both orders
    tok = ar.heads_to_tokens(x)
    assert torch.equal(ar.tokens_to_heads(tok, case.H), x)


def test_measured_constants_are_what_the_table_says():
    """C_T and C_ROT are 4 x a CPU measurement (fp32 chain against float64), never a kernel's output."""
    m = ar.measure_transcendental_constant()
    assert 0.5 * ar.C_T_MEASURED <= m <= ar.C_T_MEASURED * 1.001, m
    rot = max(ar.measure_rotation_constant(T, 32) for T in (1, 65, 256, 257, 261))
    assert 0.5 * ar.C_ROT_MEASURED <= rot <= ar.C_ROT_MEASURED * 1.001, rot
    assert ar.C_T == 4 * ar.C_T_MEASURED and ar.C_ROT == 4 * ar.C_ROT_MEASURED


PLANTED = [c for c in ar.cases() if c.BH <= 8]


@pytest.mark.parametrize("case", PLANTED, ids=str)
def test_planted_probes_are_sensitive(case):
    """Every probe, none skipped: with its one forbidden key admitted, ``out`` of the probe query moves by >= 100 x
    the forward bound in every dim, and dV of that key by >= 100 x its bound in every dim (where the key's row is
    an output at all: text padding rows and the dropped last token's row have no dV). Admitting key j for query i
    changes only row i of P, so the recomputation is of that row: exact."""
    b = ar.bundle(case, "planted")
    q, k, v, dO = b["q"], b["k"], b["v"], b["dO"]
    mask = ar.storage_mask(case)
    s2q = ar.storage_to_seq(case)
    names = {p[0] for p in b["probes"]}
    assert names >= set(ar.edges(case)), names
    if case.T % 32:
        assert "text_pad" in names
    if case.attn_type != "conv_like":   # the dropped last image token's row, across the causal / row / column edge
        assert case.Np - 1 in {sj for _, _, sj in b["probes"]}
    lanes = {si % 32 for _, si, _ in b["probes"]}
    assert {0, 31} <= lanes or case.Np < 64, lanes
    st = storage_index(case.geom, case.attn_type)
    planted = {sj for _, _, sj in b["probes"]}
    for name, cand in ar.edges(case).items():   # 8 per edge, or every key the edge has is planted (tiny grids)
        have = sum(p[0] == name for p in b["probes"])
        assert have >= ar.PROBES_PER_EDGE or all(int(st[j]) in planted for _, j in cand), (name, have)
    for name, si, sj in b["probes"]:
        assert s2q[si] >= 0 and not mask[si, sj], (name, si, sj)
        s = (q[:, si].unsqueeze(1) @ k.transpose(-1, -2)).squeeze(1)          # (BH, Np)
        allowed_max = s.masked_fill(~mask[si], -math.inf).max(dim=-1).values
        assert (s[:, sj] - allowed_max).min() >= 3.0, (name, si, sj, "score margin")
        row = mask[si].clone()
        row[sj] = True
        p = torch.softmax(s.masked_fill(~row, -math.inf), dim=-1)
        moved = ((p.unsqueeze(1) @ v).squeeze(1) - b["O"][:, si]).abs() / b["b_out"][:, si]
        assert moved.min() >= 100, (name, ar.describe_row(case, si), ar.describe_row(case, sj), moved.min().item())
        if s2q[sj] >= 0:
            moved = (p[:, sj].unsqueeze(-1) * dO[:, si]).abs() / b["b_dv"][:, sj]
            assert moved.min() >= 100, (name, ar.describe_row(case, si), ar.describe_row(case, sj), moved.min().item())


@pytest.mark.parametrize("case", [ar.Case(257, 32, "full", 5, 2, 4), ar.Case(65, 16, "axial_row", 5, 1, 3),
                                  ar.Case(40, 64, "axial_col", 5, 1, 2), ar.Case(33, 16, "conv_like", 3, 1, 3)], ids=str)
def test_ramp_crosses_the_rescale_threshold(case):
    """Per query, the running maximum over its key tiles in the order the forward visits them (ascending storage
    tile), from the reference scores in log2 units. Fast heads: every query with a second allowed tile sees at least
    one single-tile rise above RESCALE_THR. Slow heads: no single-tile rise reaches it, while the maximum still
    rises (the branch that keeps a stale maximum, P > 1). One head reaches |s| of about 60."""
    d = ar.make_ramp(case)
    r = ar.attention_ref(d["q"], d["k"], d["v"], case, mags=False)
    tm = ar.tile_running_max(r["scores"] * ar.LOG2E).reshape(case.B, case.H, case.Np, -1)[:, :, r["real"]]
    run = torch.cummax(tm, dim=-1).values
    rise = run[..., 1:] - run[..., :-1]
    rise = torch.where(torch.isfinite(run[..., :-1]), rise, torch.zeros_like(rise)).nan_to_num(0.0)   # first tile: no rise
    multi = (torch.isfinite(tm).sum(-1) >= 2)
    for h, step in enumerate(ar.ramp_heads(case)):
        top = rise[:, h].max(dim=-1).values[multi[:, h]]
        if step == ar.RAMP_FAST:
            assert (top > ar.RESCALE_THR).all(), (h, top.min().item())
        else:
            assert (rise[:, h] < ar.RESCALE_THR).all(), (h, rise[:, h].max().item())
            assert (top > 1.0).float().mean() > 0.9, h
    smax = r["scores"].masked_fill(~torch.isfinite(r["scores"]), 0.0).abs().amax(dim=(-1, -2)).reshape(case.B, case.H)
    assert 45.0 <= smax.max().item() <= 75.0, smax
