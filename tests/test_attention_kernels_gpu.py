"""K7a-e / D7: the sparse attention kernels (``attn_fwd``, ``attn_bwd``, ``attn_bwd_rope`` in its two-kernel and
one-workgroup forms, ``rope_fwd``, ``rope_bwd``) called directly on storage-layout tensors and checked element by
element against the float64 reference of ``tests/attn_ref.py`` (pinned without a GPU by ``test_attn_ref_cpu.py``).

Every kernel is judged alone: the backward kernels are given the reference's ``out`` rounded to bf16 and the
reference's ``lse`` rounded to fp32, not the forward kernel's results. Padding rows of K and V (text padding and the
dropped last image token's row) hold the finite poison 4.0 -- or, with the planted inputs, keys aligned with a real
query -- never zeros: no kernel here needs zeros in them. Padding rows of Q and dO are zero, as ``rope_fwd`` and
the token-major gather write them.

Inputs (``attn_ref.make_*``, all seeded): *random* N(0, 1.5), slice (b, h) scaled by 1 + 0.25 (b H + h) and its V
offset by 2 (b H + h) (a result from the wrong (b, h) slice -- the XCD remap at B*H = 8, 16 -- is far outside every
bound); *planted*: for every edge of every pattern >= 8 probe queries (tile lanes 0 and 31, first / last image row and
column among them), each with one forbidden key directly across the edge whose score is PLANT_SCORE = 10 and whose
value is 8 -- admitted by mistake it moves ``out`` and ``dV`` by >= 100 x the bounds below (asserted on the CPU);
*ramp*: scores rising by 3 (even heads) / 12 (odd heads) log2 units from key tile to key tile, |s| to about 60.

Bounds, from reference quantities only. u = 2^-24 (fp32), bf = 2^-8 (one rounding to bf16: 8 significant bits, so
round to nearest errs by up to 2^-8 |x| -- 1.0117 rounds to 1.0078, 2^-8.02 away; a bound of 2^-9 |x| fails the
float64 reference itself rounded to bf16, as it did here in a dry run without a GPU), P the normalised
probabilities, n_p = Np (more than the key tiles' row lengths):

    e_i    = 67 u max_j sum_d |q_id||k_jd| + C_T      relative error of one exp2: 64 fp32 accumulations of the
             exact bf16 products, the LOG2E multiply, the fma, the (stale) maximum's product, the hardware exp2
    rho_i  = 2 e_i + (n_p + 2) u + C_T                  forward P_ij / l_i before rounding (numerator, row sum of
             unrounded fp32 P, its rescales, hardware rcp)
    out    : bf |O| + (1 + bf) (bf + rho_i + n_p u) sum_j P_ij |v_jd|       P rounded to bf16 before the PV MFMA
    lse    : log2e (e_i + n_p u + C_T) + 3 u (|lse| + RESCALE_THR + log2 n_p)
    rhob_i = 67 u max_j sum_d |q||k| + ln2 u |lse_i| + C_T                    backward P_ij = exp2(s log2e - lse_i)
    dV     : bf |dV| + (1 + bf) sum_i (bf + rhob_i + n_p u) P_ij |dO_id|    P rounded to bf16 before the MFMA
    E_ij   = (bf + rhob_i + n_p u) |dS_ij| + 65 u P_ij (sum_d |dO_id||v_jd| + sum_d |dO_id||O_id|)
             dS = P (dP - delta) rounded to bf16; dP and delta (formed from the bf16 ``out`` the reference also
             reads) are 64-term fp32 sums
    dQ     : bf |dQ| + (1 + bf) sum_j E_ij |k_jd|        dK : bf |dK| + (1 + bf) sum_i E_ij |q_id|
    dqkv   : the fp32 errors above (before their bf16 rounding) through the rotation, |c| e + |s| e_partner, plus
             4 u (|c||g| + |s||g_partner|) [+ C_ROT (|g| + |g_partner|) with in-kernel angles: an angle off by d
             moves cos by d |sin| and sin by d |cos|], then bf |dqkv| for the one rounding; q's third times 1/8
    underflow: values below TINY = 2^-126, the smallest normal fp32 / bf16, are flushed to zero by exp2, the
             conversions and the MFMAs. Every bound gets + TINY; out + TINY 2^RESCALE_THR sum_j |v_jd| (a flushed
             unnormalised p over a row sum >= 2^-RESCALE_THR); dV + TINY sum_i |dO_id|; E_ij + TINY (1 + |dP_ij -
             delta_i|) -- a flushed P_ij loses dS_ij = P_ij (dP_ij - delta_i), which with large inputs is far above
             TINY itself (slices scaled by 4.75: |dP - delta| in the thousands)
    rope   : bf |y| + (1 + bf) 4 u (|c||x| + |s||x_partner|)

| constant    | value    | source                                                                        | factor |
|-------------|----------|-------------------------------------------------------------------------------|--------|
| TINY        | 2^-126   | smallest normal number of fp32 and bf16 (flush to zero below it)              |        |
| RESCALE_THR | 8        | ``attention.hip``: the running maximum may be stale by this many log2 units   |        |
| C_T_MEASURED| 6.61e-08 | ``attn_ref.measure_transcendental_constant()``: exp2 / rcp / log2 evaluated   |        |
|             |          | in fp32 against float64 on the CPU (relative; log2 relative to max(1, |.|))   |        |
| C_T         | 2.64e-07 | = 4 x C_T_MEASURED: the hardware exp2, log2, rcp                              | 4      |
| C_ROT_MEAS. | 1.66e-06 | ``attn_ref.measure_rotation_constant()``: the one-workgroup backward's        |        |
|             |          | in-kernel angle (fp32 pos x hi - rint + pos x lo) against the fp32 tables,    |        |
|             |          | cos / sin of it in float64, S = 32, T in {1, 65, 256, 257, 261}               |        |
| C_ROT       | 6.64e-06 | = 4 x C_ROT_MEASURED: that plus the hardware sin / cos                        | 4      |

Both measured constants are re-measured by ``test_attn_ref_cpu.py``; neither comes from a kernel's output.
"""
import functools

import pytest
import torch

import attn_ref as ar
from dalle_amd.models.patterns import PATTERN_IDS
from dalle_amd.models.rotary import rotary_tables

pytestmark = pytest.mark.gpu

CASES = ar.cases()
FUSED_T = [1, 65, 256, 257, 261]   # the one-workgroup backward: S = 32, axial; 261: more real keys in the 9th text tile
FUSED_CASES = [ar.Case(T, 32, at, 5, *((2, 4) if T in (65, 257) else (1, 3))) for T in FUSED_T for at in ("axial_row", "axial_col")]


@pytest.fixture(scope="module")
def ext(cuda):
    from dalle_amd.ops.ext import load_extension

    return load_extension(required=True)


@functools.lru_cache(maxsize=4)
def _bundle(case, kind, device, backward):
    return ar.bundle(case, kind, device, backward)


def bundle(case, kind, device, backward=True):
    return _bundle(case, kind, str(device), backward)


def bf16(x):
    return x.to(torch.bfloat16).contiguous()


def assert_within(got, ref, bound, case, what, rows=None):
    """Per element |got - ref| <= bound over storage-layout tensors (B*H, Np[, 64]); ``rows`` (Np,) bool selects the
    rows that are outputs (default all). Reports the worst element as slice, storage row -> position -> image
    row / col, dim."""
    got = got.detach().double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    if rows is None:
        rows = torch.ones(ref.shape[1], dtype=torch.bool, device=ref.device)
    sel = rows.view(1, -1, *([1] * (ref.dim() - 2))).expand_as(ref)
    assert torch.isfinite(got[sel]).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(sel, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    flat = int(ratio.argmax())
    d = flat % ref.shape[2] if ref.dim() == 3 else None
    rest = flat // ref.shape[2] if ref.dim() == 3 else flat
    bh, s = divmod(rest, ref.shape[1])
    bad = int(((err > bound) & sel).sum())
    msg = (f"{what} [{case}]: worst element slice (b {bh // case.H}, h {bh % case.H}), {ar.describe_row(case, s)}"
           f"{'' if d is None else f', dim {d}'}: got {got.flatten()[flat].item():.9g} ref {ref.flatten()[flat].item():.9g} "
           f"err {err.flatten()[flat].item():.3g} bound {bound.flatten()[flat].item():.3g} "
           f"(err / bound {ratio.flatten()[flat].item():.3f}); {bad} of {int(sel.sum())} elements out of bound")
    print(msg)
    assert bad == 0, msg


def tokens_to_storage(x, case):
    """token-major (B, n, H*64) -> storage (B*H, Np, 64), rows without a position zero."""
    return ar.pack(ar.tokens_to_heads(x, case.H), case)


def _args(case):
    return case.B, case.T, case.S, case.n, case.K, case.H, PATTERN_IDS[case.attn_type]


# ---------------------------------------------------------------------------------------------------------------
# rotary
ROPE_CASES = [ar.Case(T, S, at, 5, *((1, 2) if S == 64 else (2, 4) if at == "axial_col" else (1, 3)))
              for T, S in ar.GEOMS for at in ("axial_row", "axial_col")]


def _rope_inputs(case, width, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(case.B, case.n, width * case.H * 64, generator=g, dtype=torch.float64) * 1.5
    sc = (1.0 + 0.25 * torch.arange(case.BH, dtype=torch.float64)).view(case.B, 1, case.H, 1)
    x = (x.view(case.B, case.n, width * case.H, 64) * sc.repeat(1, 1, width, 1)).reshape(case.B, case.n, -1)
    return ar.bf16_round(x)


@pytest.mark.parametrize("case", ROPE_CASES, ids=str)
def test_rope_fwd_storage_layout(cuda, ext, case):
    """q (pre-scaled), k, v per element against the float64 rotation, at the storage row ``attn_ref.pack`` puts the
    token (column-major for axial_col; pinned by test_attn_ref_cpu.py::test_storage_round_trip); padding rows are
    exactly zero."""
    qkv = _rope_inputs(case, 3, 7).to(cuda)
    cos, sin = rotary_tables(case.T, case.S, 64, device=cuda)
    col = case.attn_type == "axial_col"
    got = ext.rope_fwd(bf16(qkv), cos, sin, case.T, case.S, case.H, col, ar.QSCALE)
    ref = ar.rope_fwd_ref(qkv, case)
    c64, s64 = ar.tables64(case, cuda)
    real = (ar.storage_to_seq(case) >= 0).to(cuda)
    for t, (name, x) in enumerate(zip("qkv", qkv.chunk(3, dim=-1))):
        assert got[t].shape == (case.BH, case.Np, 64) and got[t].dtype == torch.bfloat16
        mag = ar.pack(ar.apply_rotary(ar.tokens_to_heads(x.abs(), case.H), c64[:case.n].abs(), s64[:case.n].abs()), case)
        mag = mag * (ar.QSCALE if t == 0 else 1.0)
        bound = ar.BF * ref[t].abs() + (1 + ar.BF) * 4 * ar.U * mag
        assert_within(got[t], ref[t], bound, case, f"rope_fwd {name}", rows=real)
        assert (got[t][:, ~real] == 0).all(), f"rope_fwd {name}: padding rows not zero"


@pytest.mark.parametrize("case", ROPE_CASES, ids=str)
def test_rope_bwd(cuda, ext, case):
    """dqkv per element against ``apply_rotary_inverse`` of the storage-layout gradients (padding rows poisoned)."""
    g = torch.Generator().manual_seed(11)
    sc = (1.0 + 0.25 * torch.arange(case.BH, dtype=torch.float64)).view(-1, 1, 1)
    grads = [ar.bf16_round(torch.randn(case.BH, case.Np, 64, generator=g, dtype=torch.float64) * sc).to(cuda) for _ in range(3)]
    real = (ar.storage_to_seq(case) >= 0).to(cuda)
    for x in grads:
        x[:, ~real] = ar.POISON
    cos, sin = rotary_tables(case.T, case.S, 64, device=cuda)
    col = case.attn_type == "axial_col"
    got = ext.rope_bwd(*(bf16(x) for x in grads), cos, sin, case.B, case.T, case.S, case.H, case.n, col, ar.QSCALE)
    assert got.shape == (case.B, case.n, 3 * case.H * 64)
    ref = ar.rope_bwd_ref(*grads, case)
    for t, name in enumerate("qkv"):
        sl = slice(t * case.H * 64, (t + 1) * case.H * 64)
        mag = ar.rotate_bound(grads[t].abs() * (ar.QSCALE if t == 0 else 1.0), case)
        r = ref[..., sl]
        bound = ar.BF * r.abs() + (1 + ar.BF) * 4 * ar.U * mag
        assert_within(tokens_to_storage(got[..., sl].double(), case), tokens_to_storage(r, case), tokens_to_storage(bound, case),
                      case, f"rope_bwd d{name}", rows=real)


# ---------------------------------------------------------------------------------------------------------------
# forward
def _check_fwd(cuda, ext, case, kind):
    b = bundle(case, kind, cuda, backward=False)
    out, lse = ext.attn_fwd(bf16(b["q"]), bf16(b["k"]), bf16(b["v"]), *_args(case))
    assert out.shape == (case.B, case.n, case.H * 64) and lse.shape == (case.BH, case.Np)
    assert_within(tokens_to_storage(out.double(), case), b["O"], b["b_out"], case, f"attn_fwd out ({kind})", rows=b["real"])
    assert_within(lse, b["lse"], b["b_lse"], case, f"attn_fwd lse ({kind})", rows=b["real"])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_attn_fwd_elementwise(cuda, ext, case):
    """``out`` and ``lse`` per element, random inputs with slice-dependent scale and V offset."""
    _check_fwd(cuda, ext, case, "random")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_attn_fwd_planted_edges(cuda, ext, case):
    """A forbidden key across every mask edge (causal, text / pad boundary, dropped last token, axial and conv_like
    window edges): one admitted key moves ``out`` by >= 100 x the bound (and ``lse`` by log2 of its weight)."""
    _check_fwd(cuda, ext, case, "planted")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_attn_fwd_score_ramp(cuda, ext, case):
    """Scores that grow from key tile to key tile: the lazy rescale taken at every tile (odd heads) and never after
    the first (even heads, P up to 2^6 against a stale maximum); tiles wholly below the diagonal skip the mask."""
    _check_fwd(cuda, ext, case, "ramp")


# ---------------------------------------------------------------------------------------------------------------
# backward
@pytest.mark.parametrize("kind", ["random", "planted"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_attn_bwd_elementwise(cuda, ext, case, kind):
    """``attn_bwd``: dq / dk / dv in storage layout, every real row, per element. The upstream gradient of slice
    (b, h) is scaled like its inputs (random) / is +-8 on the probe queries (planted: a query admitted across an
    edge of ``query_mask`` moves that key's dV by >= 100 x the bound)."""
    b = bundle(case, kind, cuda)
    dq, dk, dv = ext.attn_bwd(bf16(b["q"]), bf16(b["k"]), bf16(b["v"]), bf16(b["out_tok"]), bf16(b["dO_tok"]),
                              b["lse32"].contiguous(), *_args(case))
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert_within(got, b["d" + name[1].upper()], b["b_" + name], case, f"attn_bwd {name} ({kind})", rows=b["real"])


def _check_bwd_rope(cuda, ext, case, kind, fused, monkeypatch):
    from dalle_amd.ops import hip_ops

    b = bundle(case, kind, cuda)
    cos, sin = rotary_tables(case.T, case.S, 64, device=cuda)
    monkeypatch.setenv("DALLE_AMD_ATTN_FUSED_BWD", "1" if fused else "0")
    got = ext.attn_bwd_rope(bf16(b["q"]), bf16(b["k"]), bf16(b["v"]), bf16(b["out_tok"]), bf16(b["dO_tok"]),
                            b["lse32"].contiguous(), cos, sin, *_args(case), ar.QSCALE, *hip_ops._rot_freqs(cuda))
    assert got.shape == (case.B, case.n, 3 * case.H * 64)
    bound = b["b_dqkv_angles" if fused else "b_dqkv_tables"]
    form = "one-workgroup" if fused else "two-kernel"
    for t, name in enumerate("qkv"):
        sl = slice(t * case.H * 64, (t + 1) * case.H * 64)
        assert_within(tokens_to_storage(got[..., sl].double(), case), tokens_to_storage(b["dqkv"][..., sl], case),
                      tokens_to_storage(bound[..., sl], case), case, f"attn_bwd_rope {form} d{name} third ({kind})", rows=b["real"])


ROPE_BWD_PARAMS = [(c, False) for c in CASES] + [(c, f) for c in FUSED_CASES for f in (False, True) if f or c not in CASES]


@pytest.mark.parametrize("kind", ["random", "planted"])
@pytest.mark.parametrize("case,fused", ROPE_BWD_PARAMS, ids=lambda v: str(v) if isinstance(v, ar.Case) else ("one-wg" if v else "two-kernel"))
def test_attn_bwd_rope_elementwise(cuda, ext, case, fused, kind, monkeypatch):
    """``attn_bwd_rope``: dqkv per element, the q, k and v thirds reported separately. The two-kernel form
    (DALLE_AMD_ATTN_FUSED_BWD=0) at every geometry; the one-workgroup form (=1, rotary angles computed in-kernel from
    ``hip_ops._rot_freqs``) at S = 32 with T in {1, 65, 256, 257, 261}. Axial patterns compute the image keys'
    dK / dV inside the dQ kernel for S <= 32 only: at S = 64 a row spans two key tiles, and the (40, 64) axial cases
    failed here (dK / dV of every row's first half) before the launcher had that condition."""
    _check_bwd_rope(cuda, ext, case, kind, fused, monkeypatch)
