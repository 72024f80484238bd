"""Persistent GEMM family (csrc/kernels/gemm_pt.hip) against fp32 PyTorch references: the plain bf16
product (+bias) and QKV + 3-axis rotary into the attention storage. Shapes cover one tile per workgroup,
several tiles per workgroup (the persistent form's continuous cross-tile DMA stream), the XCD remap
(tile count % 8 == 0) and its absence."""
import pytest
import torch

from dalle_amd.models.patterns import AttnGeometry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def test_permlane16_swap_convention(cuda):
    """The epilogues assume v_permlane16_swap trades rows 1, 3 of its first operand with rows 0, 2 of
    its second (rows = 16 lanes)."""
    from dalle_amd.ops.hip_ops import C

    out = C().permlane16_probe().cpu().tolist()
    x, y = out[:64], out[64:]
    lane = list(range(64))
    want_x = [l if (l >> 4) % 2 == 0 else 100 + l - 16 for l in lane]
    want_y = [l + 16 if (l >> 4) % 2 == 0 else 100 + l for l in lane]
    assert x == want_x and y == want_y


SHAPES = [(256, 256, 128), (512, 768, 320), (2048, 1024, 192), (4096, 2048, 256), (8192, 8192, 128), (8192, 4096, 192),
          (61440 // 8, 3072, 1024)]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("group", [0, 2, -3])
@pytest.mark.parametrize("variant", [10, 20])  # one tile per workgroup | persistent
def test_gemm_pt(cuda, M, N, K, group, variant):
    from dalle_amd.ops.hip_ops import C

    torch.manual_seed(0)
    A = torch.randn(M, K, device=cuda).bfloat16()
    B = torch.randn(N, K, device=cuda).bfloat16()
    bias = torch.randn(N, device=cuda).bfloat16()
    ref = A.float() @ B.float().t()
    got = C().gemm_pt(A, B, bias, variant, group)
    assert _rel(got, ref + bias.float()) < 5e-3
    got = C().gemm_pt(A, B, None, variant, group)
    assert _rel(got, ref) < 5e-3
    # every element is written (catch a missed tile / sub-tile): compare elementwise with a loose bound
    assert ((got.float() - ref).abs() <= 0.02 * ref.abs() + 0.5).all()
    # deterministic
    assert torch.equal(got, C().gemm_pt(A, B, None, variant, group))


def _check_qkv_rope_pt(cuda, attn_type, persist, T, B):
    from dalle_amd.ops.hip_ops import C, _rope_tables, rope_cs_table

    torch.manual_seed(0)
    S, H, D = 16, 4, 256
    geom = AttnGeometry(T, S, 5)
    n = T + S * S - 1
    h = torch.randn(B * n, D, device=cuda).bfloat16()
    w = (0.05 * torch.randn(3 * H * 64, D, device=cuda)).bfloat16()
    cos, sin = _rope_tables(geom, 64, cuda)
    col = attn_type == "axial_col"
    q, k, v = C().qkv_rope_pt(h, w, rope_cs_table(geom, 64, cuda), T, S, H, n, col, 0.125, persist)
    qkv = (h.float() @ w.float().t()).view(B, n, -1)
    # storage-layout reference: the unfused rotary kernel on the bf16-rounded product (the fused kernel
    # rotates in fp32 and rounds once, so the two differ by at most about one bf16 ulp)
    q2, k2, v2 = C().rope_fwd(qkv.bfloat16(), cos, sin, T, S, H, col, 0.125)
    for got, ref in [(q, q2), (k, k2), (v, v2)]:
        assert got.shape == ref.shape
        assert _rel(got, ref) < 1e-2
        # every element mapped (a wrong row / head / pair would be off by O(max)); rounding differences of
        # the cancelling rotary sums are bounded by the operands' scale, not the result's
        assert ((got.float() - ref.float()).abs() <= 0.02 * ref.float().abs().max()).all()


@pytest.mark.parametrize("attn_type", ["axial_row", "axial_col", "conv_like"])
@pytest.mark.parametrize("persist", [0, 1])
def test_qkv_rope_pt(cuda, attn_type, persist):
    _check_qkv_rope_pt(cuda, attn_type, persist, 65, 8)  # n = 320, M = 2560: several tiles per workgroup on small grids


@pytest.mark.parametrize("attn_type", ["axial_row", "axial_col", "conv_like"])
def test_qkv_rope_pt_n322(cuda, attn_type):
    """n = 322 (n % 16 == 2, M = 41216 = 161 * 256): rows 8 apart in a 16-row sub-tile can belong to two samples, so
    the epilogue takes its 16-row x 64-byte stores instead of whole lines -- what production runs whenever
    n % 16 != 0."""
    _check_qkv_rope_pt(cuda, attn_type, 0, 67, 128)


@pytest.mark.parametrize("cpol", [0, 1, 2, 16, 17])
@pytest.mark.parametrize("drain", [0, 1])
def test_store_policy_and_drain_bitwise(cuda, cpol, drain):
    """Output-store cache policies (gemm_set_cpol: plain / sc0 / nt / sc1 / sc0 sc1 buffer stores) and the
    end-of-workgroup store drain (gemm_set_drain) change how the epilogue writes, never what: every
    hand-written GEMM form is bitwise equal to the plain-store, no-drain result."""
    from dalle_amd.ops import hip_ops
    from dalle_amd.ops.hip_ops import rope_cs_table

    C = hip_ops.C()
    torch.manual_seed(1)
    M, N, K = 2048, 1024, 256
    A = torch.randn(M, K, device=cuda).bfloat16()
    B = torch.randn(N, K, device=cuda).bfloat16()
    bias = torch.randn(N, device=cuda).bfloat16()
    dy = (0.5 * torch.randn(M, K, device=cuda)).bfloat16()
    w2t = (0.05 * torch.randn(N, K, device=cuda)).bfloat16()
    a = torch.randn(M, 2 * N, device=cuda).bfloat16()
    # the QKV + rotary geometry of test_qkv_rope_pt
    T, S, H, D, nb = 65, 16, 4, 256, 8
    n = T + S * S - 1
    hq = torch.randn(nb * n, D, device=cuda).bfloat16()
    wq = (0.05 * torch.randn(3 * H * 64, D, device=cuda)).bfloat16()
    cs = rope_cs_table(AttnGeometry(T, S, 5), 64, cuda)

    def run_all():
        outs = [C.gemm_pt(A, B, bias, 10, 0), C.gemm_pt(A, B, bias, 20, 0), C.gemm_nt(A, B, None, 300)]
        outs += list(C.ff_dgrad_geglu(dy, w2t, a, None))
        outs += list(C.qkv_rope_pt(hq, wq, cs, T, S, H, n, False, 0.125, 0))
        return [o.clone() for o in outs]

    try:
        C.gemm_set_cpol(0)
        C.gemm_set_drain(0)
        ref = run_all()
        C.gemm_set_cpol(cpol)
        C.gemm_set_drain(drain)
        got = run_all()
    finally:
        C.gemm_set_cpol(0)
        C.gemm_set_drain(1)
    for r, g in zip(ref, got):
        assert torch.equal(r, g)
