"""Decode-step skinny GEMM (csrc/kernels/skinny.hip) and its fused epilogues vs fp32 PyTorch references
(MI355X only). Shapes cover one workgroup per column tile (KS = 1) and the cross-workgroup split-K
(last-arriver) path, and batch sizes that are not multiples of 16."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _cnt(device):
    return torch.zeros(8192, dtype=torch.int32, device=device)


SHAPES = [(64, 3072, 1024), (64, 1024, 1024), (48, 1024, 4096), (3, 768, 256), (17, 512, 384), (33, 8192, 1024)]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("f32", [False, True])
def test_skinny_linear(cuda, M, N, K, f32):
    from dalle_amd.ops.hip_ops import C

    torch.manual_seed(0)
    x = torch.randn(M, K, device=cuda).bfloat16()
    w = (0.05 * torch.randn(N, K, device=cuda)).bfloat16()
    b = torch.randn(N, device=cuda).bfloat16()
    cnt = _cnt(cuda)
    want = x.float() @ w.float().t() + b.float()
    for _ in range(3):  # counters must self-reset between launches
        got = C().skinny_linear(x, w, b, f32, cnt)
        assert got.dtype == (torch.float32 if f32 else torch.bfloat16)
        assert _rel(got, want) < 1e-2
    assert int(cnt.abs().sum()) == 0
    got = C().skinny_linear(x, w, None, f32, cnt)
    assert _rel(got, x.float() @ w.float().t()) < 1e-2


def test_skinny_deterministic(cuda):
    from dalle_amd.ops.hip_ops import C

    torch.manual_seed(0)
    x = torch.randn(64, 4096, device=cuda).bfloat16()
    w = torch.randn(1024, 4096, device=cuda).bfloat16()
    cnt = _cnt(cuda)
    a = C().skinny_linear(x, w, None, True, cnt)
    for _ in range(5):
        assert torch.equal(C().skinny_linear(x, w, None, True, cnt), a)


@pytest.mark.parametrize("M,F,K", [(64, 4096, 1024), (5, 1024, 256)])
def test_skinny_geglu(cuda, M, F, K):
    from dalle_amd.ops.hip_ops import C

    torch.manual_seed(0)
    x = torch.randn(M, K, device=cuda).bfloat16()
    w = (0.05 * torch.randn(2 * F, K, device=cuda)).bfloat16()
    b = torch.randn(2 * F, device=cuda).bfloat16()
    y = x.float() @ w.float().t() + b.float()
    a, g = y.chunk(2, -1)
    want = a * torch.nn.functional.gelu(g)
    got = C().skinny_geglu(x, w, b, _cnt(cuda))
    assert got.shape == (M, F)
    assert _rel(got, want) < 1e-2


@pytest.mark.parametrize("M,N,K", [(64, 1024, 4096), (64, 1024, 1024), (7, 256, 1024)])
def test_skinny_residual(cuda, M, N, K):
    from dalle_amd.ops.hip_ops import C

    torch.manual_seed(0)
    x = torch.randn(M, K, device=cuda).bfloat16()
    w = (0.05 * torch.randn(N, K, device=cuda)).bfloat16()
    b = torch.randn(N, device=cuda).bfloat16()
    scale = torch.rand(N, device=cuda)
    res = torch.randn(M, N, device=cuda)
    want = res + scale * (x.float() @ w.float().t() + b.float())
    C().skinny_residual_(res, x, w, b, scale, _cnt(cuda))
    assert _rel(res, want) < 1e-3


@pytest.mark.parametrize("M,H", [(64, 16), (3, 4)])
def test_skinny_qkv_rope(cuda, M, H):
    from dalle_amd.ops.hip_ops import C
    from dalle_amd.models.rotary import rotary_tables

    torch.manual_seed(0)
    K, T, S = 64 * H, 17, 8
    n = T + S * S - 1
    cos, sin = rotary_tables(T, S, 64, device=cuda)
    x = torch.randn(M, K, device=cuda).bfloat16()
    w = (0.05 * torch.randn(3 * H * 64, K, device=cuda)).bfloat16()
    pos = torch.tensor(T + 11, dtype=torch.int32, device=cuda)
    q = torch.zeros(M * H, 64, dtype=torch.bfloat16, device=cuda)
    kc = torch.zeros(M * H, n, 64, dtype=torch.bfloat16, device=cuda)
    vc = torch.zeros_like(kc)
    C().skinny_qkv_rope_(x, w, cos, sin, q, kc, vc, pos, H, 0.125, _cnt(cuda))
    # reference: the unfused decode path (GEMM then the decode rotary kernel)
    q2, kc2, vc2 = torch.zeros_like(q), torch.zeros_like(kc), torch.zeros_like(vc)
    qkv = (x.float() @ w.float().t()).bfloat16()
    C().decode_rope_(qkv, cos, sin, q2, kc2, vc2, pos, H, 0.125)
    assert _rel(q, q2) < 1e-2
    assert _rel(kc, kc2) < 1e-2 and _rel(vc, vc2) < 1e-2
    p = int(pos)
    assert kc[:, :p].abs().sum() == 0 and kc[:, p + 1:].abs().sum() == 0
    # past the cache end: no write at all
    pos.fill_(n)
    kc.zero_()
    C().skinny_qkv_rope_(x, w, cos, sin, q, kc, vc, pos, H, 0.125, _cnt(cuda))
    assert kc.abs().sum() == 0


@pytest.mark.parametrize("M,N,K,slabs", [(3, 48, 256, 1), (17, 512, 384, 3), (33, 256, 1024, 4), (64, 1024, 4096, 8)])
def test_skinny_partials(cuda, M, N, K, slabs):
    """The split-K slabs the decode step's QKV / out-proj / FF-out projections leave (skinny EPI 4): all three
    M-block counts, 1 / 2 / 4 waves per workgroup, a row count that is no multiple of 16. bf16 x bf16 products are
    exact in fp32, so only the K additions round: elementwise |sum_k part[k] - ref| <= 2 K 2^-24 (|x| @ |w|^T)
    against float64 (the 2 covers a truncating accumulator as well as round-to-nearest)."""
    from dalle_amd.ops.hip_ops import C

    torch.manual_seed(0)
    x = torch.randn(M, K, device=cuda).bfloat16()
    w = (0.05 * torch.randn(N, K, device=cuda)).bfloat16()
    part = C().skinny_partials(x, w)
    assert part.shape == (slabs, M, N) and part.dtype == torch.float32  # (M, N) per slab: no padded rows exist
    ref = x.double() @ w.double().t()
    bound = 2 * K * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t())
    err = (part.double().sum(0) - ref).abs()
    print(f"skinny_partials {(M, N, K)}: {slabs} slabs, largest error / bound = {(err / bound).max().item():.3e}")
    assert (err <= bound).all()
    for _ in range(3):
        assert torch.equal(C().skinny_partials(x, w), part)


LN_T, LN_S = 17, 8
LN_N = LN_T + LN_S * LN_S - 1


def _ln_shift_ref(xn, w, b, hist, pos, shift):
    """DecodeEngine._ln_shift's CPU branch in float64: the LN row (the history row at ``pos``) and the shifted row."""
    D = xn.shape[-1]
    y = torch.nn.functional.layer_norm(xn, (D,), w, b, 1e-5)
    out = y.clone()
    if shift:
        q, h2 = D // 4, D // 2
        if pos < LN_T:
            out[:, :h2] = hist[:, pos - 1, :h2] if pos >= 1 else 0.0
        else:
            k = pos - LN_T
            out[:, :q] = hist[:, pos - LN_S, :q] if k >= LN_S else 0.0
            out[:, q:h2] = hist[:, pos - 1, q:h2] if k % LN_S else 0.0
    return y, out


@pytest.mark.parametrize("KS", [1, 3, 16])
@pytest.mark.parametrize("D", [256, 1024])
def test_slab_consumers(cuda, D, KS):
    """The kernels that apply a pending residual update x += scale * (sum of slabs + bias): residual_from_partials_
    and decode_ln_shift_ with pending slabs (one wave per row and four; 16 slabs is the binding's cap), with and
    without bias, at a text position with no shift source (0) and with one (5), the first image token (both
    sources absent), the first column of the second image row (upper source only) and a position with both.
    x within the fp32 rounding of KS - 1 slab additions, the bias, the scale and the residual addition (KS + 3
    covers them) against float64; LN history row and output within the project's bf16 LayerNorm bound (0.05 at
    test_prefill_kernels_match_torch's input scales: half a bf16 ulp below 16 is 0.031)."""
    from dalle_amd.ops.hip_ops import C

    g = torch.Generator().manual_seed(0)
    B, n = 3, LN_N
    x0 = (torch.randn(B, D, generator=g) * 2 + 0.5).to(cuda)
    w, b = torch.randn(D, generator=g).to(cuda), torch.randn(D, generator=g).to(cuda)
    scale = torch.rand(D, generator=g).to(cuda)
    bias = torch.randn(D, generator=g).bfloat16().to(cuda)
    part = torch.randn(KS, B, D, generator=g).to(cuda)
    hist0 = torch.randn(B, n, D, generator=g).bfloat16().to(cuda)
    for pb in (bias, None):
        pb64 = pb.double() if pb is not None else torch.zeros(D, dtype=torch.float64, device=cuda)
        xn = x0.double() + scale.double() * (part.double().sum(0) + pb64)
        xbound = (KS + 3) * 2.0 ** -24 * (x0.double().abs() + scale.double().abs() * (part.double().abs().sum(0) + pb64.abs()))
        x = x0.clone()
        C().residual_from_partials_(x, part, pb, scale)
        assert ((x.double() - xn).abs() <= xbound).all()
        for pos in (0, 5, LN_T, LN_T + LN_S, LN_T + LN_S + 3):
            for shift in (True, False):
                x, hist = x0.clone(), hist0.clone()
                y = torch.zeros(B, D, dtype=torch.bfloat16, device=cuda)
                p = torch.tensor(pos, dtype=torch.int32, device=cuda)
                C().decode_ln_shift_(x, w, b, hist, y, p, LN_T, LN_S, shift, part, pb, scale)
                ry, rout = _ln_shift_ref(xn, w.double(), b.double(), hist0.double(), pos, shift)
                assert ry.abs().max().item() < 16  # the inputs: where 0.05 is above the bf16 rounding
                assert ((x.double() - xn).abs() <= xbound).all()
                assert (hist[:, pos].double() - ry).abs().max().item() < 0.05
                assert (y.double() - rout).abs().max().item() < 0.05
                hist[:, pos] = hist0[:, pos]
                assert torch.equal(hist, hist0)  # no other history row touched
        # past the cache end: the kernel returns before its first load
        x, hist = x0.clone(), hist0.clone()
        y = torch.zeros(B, D, dtype=torch.bfloat16, device=cuda)
        C().decode_ln_shift_(x, w, b, hist, y, torch.tensor(n, dtype=torch.int32, device=cuda), LN_T, LN_S, True, part, pb, scale)
        assert torch.equal(x, x0) and torch.equal(hist, hist0) and y.abs().sum().item() == 0


def _attn_part_case(cuda, KS, T, S, Ks, pattern, positions):
    """decode_attn_part_ (q / k / v summed from the QKV slabs in the attention's prologue) against the path it
    replaces: decode_rope_ on the slab sum rounded to bf16, then decode_attn_."""
    from dalle_amd.models.patterns import PATTERN_IDS
    from dalle_amd.models.rotary import rotary_tables
    from dalle_amd.ops.hip_ops import C

    torch.manual_seed(0)
    B, H = 3, 4
    n = T + S * S - 1
    cos, sin = rotary_tables(T, S, 64, device=cuda)
    part = torch.randn(KS, B, 3 * H * 64, device=cuda)
    kc0 = torch.randn(B * H, n, 64, device=cuda).bfloat16()
    vc0 = torch.randn(B * H, n, 64, device=cuda).bfloat16()
    qkv = part.sum(0).bfloat16()
    for pos in positions:
        pos = n - 1 if pos is None else pos
        p = torch.tensor(pos, dtype=torch.int32, device=cuda)
        kc, vc = kc0.clone(), vc0.clone()
        out = torch.zeros(B, H * 64, dtype=torch.bfloat16, device=cuda)
        C().decode_attn_part_(part, cos, sin, 0.125, kc, vc, out, p, T, S, H, Ks, PATTERN_IDS[pattern])
        q2 = torch.zeros(B * H, 64, dtype=torch.bfloat16, device=cuda)
        kc2, vc2, out2 = kc0.clone(), vc0.clone(), torch.zeros_like(out)
        C().decode_rope_(qkv, cos, sin, q2, kc2, vc2, p, H, 0.125)
        C().decode_attn_(q2, kc2, vc2, out2, p, T, S, H, Ks, PATTERN_IDS[pattern])
        assert _rel(out, out2) < 1e-2, (pattern, pos)
        assert _rel(kc[:, pos], kc2[:, pos]) < 1e-2 and _rel(vc[:, pos], vc2[:, pos]) < 1e-2
        kc[:, pos], vc[:, pos] = kc0[:, pos], vc0[:, pos]
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0)  # no other cache row touched


@pytest.mark.parametrize("pattern", ["full", "axial_row", "axial_col", "conv_like"])
@pytest.mark.parametrize("KS", [1, 3])
def test_decode_attn_part(cuda, KS, pattern):
    """A text position, image positions in the first and second row, and the last position of the sequence."""
    T, S = 17, 8
    _attn_part_case(cuda, KS, T, S, 5, pattern, (5, T + 3, T + 11, None))


@pytest.mark.parametrize("KS", [1, 3])
def test_decode_attn_part_long_full(cuda, KS):
    """Full attention over 301 and 1101 keys: up to and past one 320-key chunk (the chunked two-pass path)."""
    _attn_part_case(cuda, KS, 257, 32, 11, "full", (300, 1100))


@pytest.mark.parametrize("pattern,pos", [("full", 1100), ("full", 300), ("axial_row", 1000), ("axial_col", 900),
                                         ("conv_like", 700), ("axial_row", 100)])
def test_decode_attention_kernel(cuda, pattern, pos):
    """Decode attention (single-chunk and chunked paths) vs an fp32 softmax over the static mask row."""
    from dalle_amd.models.patterns import AttnGeometry, PATTERN_IDS, static_mask
    from dalle_amd.ops.hip_ops import C

    torch.manual_seed(0)
    T, S, H, B, Ks = 257, 32, 4, 3, 11
    n = T + S * S - 1
    geom = AttnGeometry(T, S, Ks)
    q = torch.randn(B * H, 64, device=cuda).bfloat16()
    kc = torch.randn(B * H, n, 64, device=cuda).bfloat16()
    vc = torch.randn(B * H, n, 64, device=cuda).bfloat16()
    out = torch.zeros(B, H * 64, dtype=torch.bfloat16, device=cuda)
    p = torch.tensor(pos, dtype=torch.int32, device=cuda)
    C().decode_attn_(q, kc, vc, out, p, T, S, H, Ks, PATTERN_IDS[pattern])
    mask = static_mask(geom, pattern, n, device=cuda)[pos, : pos + 1]
    sc = (q.float()[:, None, :] @ kc[:, : pos + 1].float().transpose(1, 2))[:, 0]
    sc = sc.masked_fill(~mask, float("-inf"))
    want = (torch.softmax(sc, -1)[:, None, :] @ vc[:, : pos + 1].float())[:, 0]
    assert _rel(out.view(B * H, 64), want) < 1e-2
