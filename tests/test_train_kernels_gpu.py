"""K1-K4, K8 / K10, K9, K12: the residual-stream training kernels (``ln_shift_fwd``, ``ln_shift_fwd_res``,
``ln_shift_bwd``, ``ln_shift_bwd_sr``, ``geglu_fwd``, ``geglu_bwd``, ``geglu_bwd_bias``, ``scale_residual_``,
``scale_residual_out``, ``scale_residual_bwd``, ``xent_fwd_bwd_``, ``xent_colsum_``, ``embed_fwd``, ``embed_bwd_``) called
directly and checked element by element against the float64 references of ``tests/train_ref.py`` (pinned without a
GPU by ``test_train_ref_cpu.py``, which also passes an fp32 emulation of each kernel through every bound below and
shows planted defects >= 10 x outside them). Every element of every output is checked; nothing is excluded.

Every kernel is judged alone: the LayerNorm backward is given the reference's ``mean`` / ``rstd`` rounded to fp32 and
the boundary backward the reference's ``xout`` rounded to fp32, not the forward kernels' results. Results whose
positions nobody may skip (``y`` with its owed zeros, ``dx``, ``dyprev``) are written over NaN: immediately before the
call a bf16 tensor of the output's size in bytes is filled with NaN and freed (one per output the binding allocates
before it, in the binding's order), and the result must land on its address -- asserted, or the poison proves nothing.
Sinks hold non-zero prior content; ``after - before`` is checked. Every backward runs twice, bitwise equal.

Bounds, from reference quantities only. u = 2^-24, bf = 2^-8 (one rounding to bf16), TINY = 2^-126, d = D / 64 + 6
(the additions a term of a row sum passes through: D / 64 per lane in sequence, then the 6-level butterfly):

    mean   : d u mean|x| + u |mean|                                   (+ mean e_x: the boundary's fp32 x, below)
    var    : (d + 4) u var + b_mean^2 (+ mean(2 |x - m| e_x + e_x^2))   sum (x - m^)^2 = sum (x - m)^2 + D (m - m^)^2:
             the mean's error enters squared; the centred squares cost 3 roundings, their sum d, the 1 / D none
    rstd   : rstd (var error / (2 (var + eps)) + C_RSQRT + 2 u)          eps as fp32, the add, the hardware rsqrt
    y      : bf |y| + (1 + bf) e_y + TINY,  e_y = |w| (rstd (b_mean + e_x + u |x - m|) + |x - m| b_rstd)
             + 3 u |(x - m) rstd w| + u |y|;  exactly 0 where zeros are owed
    xout   : e_x = 2 u (|res| + |sprev yprev|)                           one fused or unfused multiply-add
    dx     : rstd (u |gy| + e_s1 + |xh| e_s2 + 3 u |xh| |s2|) + 4 u rstd (|gy| + |s1| + |xh s2|) + u |dx| + u |resid|
             gy = g w, xh = (x - mean) rstd (3 u |xh|), s1 = mean gy: e_s1 = (d + 1) u mean|gy|,
             s2 = mean gy xh: e_s2 = (d + 2) u mean|gy xh| + mean(|gy| 3 u |xh|)
    dw, db : (rows + 1) u sum|g xh| + sum |g| 3 u |xh|;  rows u sum|g|       fixed but unspecified order
    dyprev : bf |.| + (1 + bf) (|sprev| e_dx + u |.|) + TINY
    dscale_prev : (rows + 1) u sum|dx yprev| + sum e_dx |yprev|;   dbias_prev : |sprev| (rows u sum|dx| + sum e_dx) + u |.|
    geglu fwd : bf |out| + (1 + bf) (|a| e_gelu + u |out|) + TINY,  e_gelu = |g| / 2 (erf'(z) 2 u |z| + C_ERF |erf| +
             u (1 + |erf|)) + 2 u |gelu|, z = g / sqrt 2 (absolute in the negative tail, where 1 + erf cancels)
    geglu bwd : e_cdf = (C_AS_FORMULA + C_AS_EVAL) / 2 + u: absolute, so da: bf |da| + (1 + bf) (|d| (|g| e_cdf + u |gelu|)
             + u |da|) + TINY and dg: bf |dg| + (1 + bf) (|d a| (e_cdf + |g| pdf(g) (2 u g^2 + 2 u + C_T) + u |gelu'|) +
             2 u |dg|) + TINY (the exponent -g^2 log2e / 2 has 3 roundings; the hardware exp2)
    bias sums : against the float64 column sums of the bf16 values the kernel itself stored: rows u sum|.| (geglu, xent)
    xent   : term j of the row sum is exp2((f_j - m) log2e) through K = ceil(V / 2048) + 3 evaluations (the online
             forms rescale by exp(m_old - m_new); the exponents telescope to |f_j - M|, each with 3 roundings:
             the subtraction, the constant log2e, the product) and N = 8 ceil(V / 2048) + 32 additions:
             e_S = sum_j p_j 3 u |f_j - M| + K (3 u + C_T) + N u          relative, of the sum
             lse  : e_S + (C_T + 2 u) max(1, |log2 S|) + u |lse|;   loss : that + u (|lse| + |loss|)
             dlogits : bf |G| + (1 + bf) (gscale p (3 u |f - lse| + 2 u + C_T + b_lse + u |lse|) + 2 u |G|) + TINY;
             the padding columns (logit -3e4) are asserted exactly 0, and so are their bias increments
    scale_residual : 2 u (|x| + |s y|);  bwd dy : bf |.| + (1 + bf) u |.| + TINY; dscale : (M + 1) u sum|g y|; gsum : M u sum|g|
    embed_fwd : exact;  embed_bwd_ : (run length + 1) u (sum|rows| + |before|)
    sinks  : + 2 u (|before| + |ref|) for the add into the prior content

| constant          | value    | source                                                                   | factor |
|-------------------|----------|--------------------------------------------------------------------------|--------|
| C_T_MEASURED      | 6.61e-08 | ``attn_ref.measure_transcendental_constant()`` (exp2 / rcp / log2)       |        |
| C_T               | 2.64e-07 | = 4 x C_T_MEASURED: the hardware exp2, log2, rcp                         | 4      |
| C_RSQRT_MEASURED  | 8.81e-08 | ``train_ref.measure_rsqrt_constant()``: rsqrt in fp32 against float64    |        |
| C_RSQRT           | 3.52e-07 | = 4 x C_RSQRT_MEASURED: the hardware rsqrt                               | 4      |
| C_ERF_MEASURED    | 5.99e-08 | ``train_ref.measure_erff_constant()``: erff in fp32 against float64      |        |
| C_ERF             | 2.40e-07 | = 4 x C_ERF_MEASURED: ocml erff (relative)                               | 4      |
| C_AS_FORMULA      | 1.5e-07  | Abramowitz-Stegun 7.1.26's own absolute error on erf (the handbook's     |        |
|                   |          | figure; ``measure_as_constants()[0]`` = 1.39e-07 in float64 is below it) |        |
| C_AS_EVAL_MEASURED| 3.44e-07 | ``measure_as_constants()[1]``: ``gelu_and_grad``'s polynomial, rcp and   |        |
|                   |          | exp2 in fp32 on the CPU against their float64 evaluation, |x| <= 14      |        |
| C_AS_EVAL         | 1.38e-06 | = 4 x C_AS_EVAL_MEASURED (absolute, on erf)                              | 4      |

All measured constants are re-measured by ``test_train_ref_cpu.py``; none comes from a kernel's output.
"""
import pytest
import torch

import train_ref as tr

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ext(cuda):
    from dalle_amd.ops.ext import load_extension

    return load_extension(required=True)


def assert_within(got, ref, bound, what):
    """Per element |got - ref| <= bound (a bound of 0 demands equality). Reports the worst element's coordinates,
    err / bound and the count out of bound."""
    got = got.detach().double().reshape(ref.shape)
    assert ref.shape == bound.shape, (what, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output ({int((~torch.isfinite(got)).sum())} elements)"
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape)) if ref.dim() else ()
    bad = int((err > bound).sum())
    msg = (f"{what}: worst element {idx}: got {got.flatten()[flat].item():.9g} ref {ref.flatten()[flat].item():.9g} "
           f"err {err.flatten()[flat].item():.3g} bound {bound.flatten()[flat].item():.3g} "
           f"(err / bound {min(ratio.flatten()[flat].item(), 1e99):.3f}); {bad} of {ref.numel()} elements out of bound")
    print("[within]", msg)
    assert bad == 0, msg


def poison(device, *nbytes):
    """NaN-filled bf16 tensors of the given sizes in bytes, allocated in order and freed: -> their addresses, which the
    caching allocator hands to the next allocations of the same sizes in the same order."""
    ts = [torch.full((nb // 2,), NAN, dtype=torch.bfloat16, device=device) for nb in nbytes]
    ptrs = [t.data_ptr() for t in ts]
    del ts
    return ptrs


def landed(t, ptr, what):
    assert t.data_ptr() == ptr, f"{what}: the result did not land on the NaN-filled block; the poison proves nothing"


def f32(x, dev):
    return x.to(torch.float32).to(dev).contiguous()


def b16(x, dev):
    return x.to(torch.bfloat16).to(dev).contiguous()


def sink_check(after, before, ref, bound, what):
    assert_within(after.double() - before.double(), ref, bound + tr.sink_slack(before.double(), ref), what)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm + token shift
LN_CASES = [(D, *g, 3) for D in (256, 512, 1024, 2048) for g in tr.LN_GEOMS]
LN_CASES += [(256, 1, 8, 1, True, 1),          # B = 1, n = 1
             (256, 9, 32, 1032, True, 2),      # 2064 rows: the backward's 512-block cap gives waves a second row
             (256, 9, 32, 1032, True, 4)]      # 4128 rows: and a third, through the prefetch pipeline
ln_id = lambda c: "D{}-T{}-S{}-n{}-{}-B{}".format(c[0], c[1], c[2], c[3], "shift" if c[4] else "plain", c[5])  # noqa: E731


@pytest.mark.parametrize("case", LN_CASES, ids=ln_id)
def test_ln_shift_fwd(cuda, ext, case):
    """mean, rstd and every element of y (owed zeros exactly 0, written over NaN) for each input kind."""
    D, T, S, n, shift, B = case
    w, b = (t.to(cuda) for t in tr.ln_params(D))
    for kind in tr.LN_KINDS:
        x = tr.ln_rows(kind, B, n, D).to(cuda)
        r = tr.ln_shift_ref(x, w, b, T, S, n, shift)
        xg, wg, bg = f32(x, cuda), f32(w, cuda), f32(b, cuda)
        (ptr,) = poison(cuda, B * n * D * 2)
        y, mean, rstd = ext.ln_shift_fwd(xg, wg, bg, T, S, shift, tr.EPS)
        landed(y, ptr, "ln_shift_fwd y")
        assert_within(mean, r["mean"], r["b_mean"], f"ln_shift_fwd mean [{ln_id(case)} {kind}]")
        assert_within(rstd, r["rstd"], r["b_rstd"], f"ln_shift_fwd rstd [{ln_id(case)} {kind}]")
        assert_within(y, r["y"], r["b_y"], f"ln_shift_fwd y [{ln_id(case)} {kind}]")


@pytest.mark.parametrize("case", LN_CASES, ids=ln_id)
def test_ln_shift_bwd(cuda, ext, case):
    """dx (with and without the residual-stream gradient, written over NaN), dw, db returned and accumulated into
    pre-filled sinks; two runs bitwise equal."""
    D, T, S, n, shift, B = case
    w, b = (t.to(cuda) for t in tr.ln_params(D))
    wg = f32(w, cuda)
    for ki, kind in enumerate(tr.LN_KINDS):
        tag = f"[{ln_id(case)} {kind}]"
        x = tr.ln_rows(kind, B, n, D).to(cuda)
        fwd = tr.ln_shift_ref(x, w, b, T, S, n, shift)
        m32, r32 = tr.f32_round(fwd["mean"]), tr.f32_round(fwd["rstd"])
        dy = tr.randn_bf16((B, n, D), 1.0, 700 + ki).to(cuda)
        resid = tr.randn_f32((B, n, D), 1.0, 710 + ki).to(cuda)
        xg, dyg, mg, rg, resg = f32(x, cuda), b16(dy, cuda), f32(m32, cuda), f32(r32, cuda), f32(resid, cuda)
        q = tr.ln_shift_bwd_ref(x, w, dy, m32, r32, fwd["map"], resid=resid)
        (ptr,) = poison(cuda, B * n * D * 4)
        dx, dw, db = ext.ln_shift_bwd(xg, wg, dyg, mg, rg, T, S, shift, resg)
        landed(dx, ptr, "ln_shift_bwd dx")
        assert_within(dx, q["dx"], q["b_dx"], f"ln_shift_bwd dx +resid {tag}")
        assert_within(dw, q["dw"], q["b_dw"], f"ln_shift_bwd dw {tag}")
        assert_within(db, q["db"], q["b_db"], f"ln_shift_bwd db {tag}")
        dx2, dw2, db2 = ext.ln_shift_bwd(xg, wg, dyg, mg, rg, T, S, shift, resg)
        assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2), f"not deterministic {tag}"
        # no residual gradient, sinks with prior content
        q0 = tr.ln_shift_bwd_ref(x, w, dy, m32, r32, fwd["map"])
        gw0, gb0 = f32(tr.randn_f32((D,), 3.0, 720), cuda), f32(tr.randn_f32((D,), 3.0, 721), cuda)
        gw, gb = gw0.clone(), gb0.clone()
        (ptr,) = poison(cuda, B * n * D * 4)
        dx3, none_w, none_b = ext.ln_shift_bwd(xg, wg, dyg, mg, rg, T, S, shift, None, gw, gb)
        landed(dx3, ptr, "ln_shift_bwd dx (sinks)")
        assert none_w is None and none_b is None
        assert_within(dx3, q0["dx"], q0["b_dx"], f"ln_shift_bwd dx {tag}")
        sink_check(gw, gw0, q0["dw"], q0["b_dw"], f"ln_shift_bwd dw sink {tag}")
        sink_check(gb, gb0, q0["db"], q0["b_db"], f"ln_shift_bwd db sink {tag}")


BOUNDARY_CASES = [(D, T, S, n, True, 3) for D in (256, 1024, 2048) for T, S, n in ((9, 8, 72), (65, 16, 320))]
BOUNDARY_CASES += [(256, 9, 32, 1032, True, 4)]


def _boundary_inputs(case, kind, dev):
    D, T, S, n, shift, B = case
    res = tr.ln_rows(kind, B, n, D).to(dev)
    yprev = tr.randn_bf16((B, n, D), 1.0, 730).to(dev)
    sprev = tr.sprev_vector(D).to(dev)
    w, b = (t.to(dev) for t in tr.ln_params(D))
    return res, yprev, sprev, w, b


@pytest.mark.parametrize("case", BOUNDARY_CASES, ids=ln_id)
def test_ln_shift_fwd_res(cuda, ext, case):
    """The fused boundary, forward: xout = res + sprev * yprev, its mean / rstd and shifted y (over NaN)."""
    D, T, S, n, shift, B = case
    for kind in tr.LN_KINDS:
        tag = f"[{ln_id(case)} {kind}]"
        res, yprev, sprev, w, b = _boundary_inputs(case, kind, cuda)
        r = tr.boundary_fwd_ref(res, yprev, sprev, w, b, T, S, n, shift)
        args = f32(res, cuda), b16(yprev, cuda), f32(sprev, cuda), f32(w, cuda), f32(b, cuda)
        px, py = poison(cuda, B * n * D * 4, B * n * D * 2)
        xout, y, mean, rstd = ext.ln_shift_fwd_res(*args, T, S, shift, tr.EPS)
        landed(xout, px, "ln_shift_fwd_res xout")
        landed(y, py, "ln_shift_fwd_res y")
        assert_within(xout, r["xout"], r["b_xout"], f"ln_shift_fwd_res xout {tag}")
        assert_within(mean, r["mean"], r["b_mean"], f"ln_shift_fwd_res mean {tag}")
        assert_within(rstd, r["rstd"], r["b_rstd"], f"ln_shift_fwd_res rstd {tag}")
        assert_within(y, r["y"], r["b_y"], f"ln_shift_fwd_res y {tag}")


@pytest.mark.parametrize("case", BOUNDARY_CASES, ids=ln_id)
def test_ln_shift_bwd_sr(cuda, ext, case):
    """The fused boundary, backward: dx and dyprev (over NaN), and the four pre-filled sinks (dw, db of this
    sublayer; dscale_prev, dbias_prev = sprev * sum dx of the previous one, through the two-task column sum)."""
    D, T, S, n, shift, B = case
    for ki, kind in enumerate(tr.LN_KINDS):
        tag = f"[{ln_id(case)} {kind}]"
        res, yprev, sprev, w, b = _boundary_inputs(case, kind, cuda)
        x = tr.f32_round(res + sprev * yprev)
        fwd = tr.ln_shift_ref(x, w, b, T, S, n, shift)
        m32, r32 = tr.f32_round(fwd["mean"]), tr.f32_round(fwd["rstd"])
        dy = tr.randn_bf16((B, n, D), 1.0, 740 + ki).to(cuda)
        resid = tr.randn_f32((B, n, D), 1.0, 750 + ki).to(cuda)
        q = tr.ln_shift_bwd_ref(x, w, dy, m32, r32, fwd["map"], resid=resid, yprev=yprev, sprev=sprev)
        args = (f32(x, cuda), f32(w, cuda), b16(dy, cuda), f32(m32, cuda), f32(r32, cuda), T, S, shift, f32(resid, cuda),
                b16(yprev, cuda), f32(sprev, cuda))
        before = [f32(tr.randn_f32((D,), 3.0, 760 + i), cuda) for i in range(4)]
        sinks = [t.clone() for t in before]
        pdx, pdy = poison(cuda, B * n * D * 4, B * n * D * 2)
        dx, dyp = ext.ln_shift_bwd_sr(*args, *sinks)
        landed(dx, pdx, "ln_shift_bwd_sr dx")
        landed(dyp, pdy, "ln_shift_bwd_sr dyprev")
        assert_within(dx, q["dx"], q["b_dx"], f"ln_shift_bwd_sr dx {tag}")
        assert_within(dyp, q["dyprev"], q["b_dyprev"], f"ln_shift_bwd_sr dyprev {tag}")
        for s, s0, name in zip(sinks, before, ("dw", "db", "dscale_prev", "dbias_prev")):
            sink_check(s, s0, q[name], q["b_" + name], f"ln_shift_bwd_sr {name} sink {tag}")
        sinks2 = [t.clone() for t in before]
        dx2, dyp2 = ext.ln_shift_bwd_sr(*args, *sinks2)
        assert torch.equal(dx, dx2) and torch.equal(dyp, dyp2), f"not deterministic {tag}"
        assert all(torch.equal(a, c) for a, c in zip(sinks, sinks2)), f"sinks not deterministic {tag}"


# ---------------------------------------------------------------------------------------------------------------
# GEGLU
@pytest.mark.parametrize("M,F", tr.GEGLU_SHAPES)
def test_geglu(cuda, ext, M, F):
    """geglu_fwd (ocml erff), geglu_bwd and geglu_bwd_bias (the Abramowitz-Stegun erf) per element; the bias sums
    against the float64 column sums of the stored dh, returned and accumulated into a pre-filled sink."""
    tag = f"[M {M} F {F}]"
    h16, h, d = tr.geglu_inputs(M, F)
    hg, dg = h16.to(cuda).contiguous(), b16(d, cuda)
    h, d = h.to(cuda), d.to(cuda)
    ref, bound = tr.geglu_fwd_ref(h)
    assert_within(ext.geglu_fwd(hg), ref, bound, f"geglu_fwd {tag}")
    ref, bound = tr.geglu_bwd_ref(h, d)
    (ptr,) = poison(cuda, M * 2 * F * 2)
    dh = ext.geglu_bwd(hg, dg)
    landed(dh, ptr, "geglu_bwd dh")
    assert_within(dh, ref, bound, f"geglu_bwd {tag}")
    assert torch.equal(dh, ext.geglu_bwd(hg, dg)), "geglu_bwd not deterministic"
    (ptr,) = poison(cuda, M * 2 * F * 2)
    dh1, db1 = ext.geglu_bwd_bias(hg, dg)
    landed(dh1, ptr, "geglu_bwd_bias dh")
    assert_within(dh1, ref, bound, f"geglu_bwd_bias dh {tag}")
    s, sb = tr.column_sum_check(dh1)
    assert_within(db1, s, sb, f"geglu_bwd_bias db {tag}")
    gb0 = f32(tr.randn_f32((2 * F,), 3.0, 770), cuda)
    gb = gb0.clone()
    dh2, none_b = ext.geglu_bwd_bias(hg, dg, gb)
    assert none_b is None and torch.equal(dh1, dh2), "geglu_bwd_bias not deterministic"
    sink_check(gb, gb0, s, sb, f"geglu_bwd_bias db sink {tag}")
    gb2 = gb0.clone()
    ext.geglu_bwd_bias(hg, dg, gb2)
    assert torch.equal(gb, gb2) and torch.equal(db1, ext.geglu_bwd_bias(hg, dg)[1]), "bias sums not deterministic"


# ---------------------------------------------------------------------------------------------------------------
# LayerScale residual
@pytest.mark.parametrize("D", [8, 256, 776, 1024, 2048])
def test_scale_residual(cuda, ext, D):
    """scale_residual_ in place and scale_residual_out; the backward's dy, dscale, gsum returned and accumulated into
    pre-filled sinks (gbias += scale * sum g), for 256 / (D / 8) rows per iteration and a D / 8 that does not divide 256."""
    for M in (1, 77, 1030):
        tag = f"[M {M} D {D}]"
        x, y, s = tr.randn_f32((M, D), 2.0, 780).to(cuda), tr.randn_bf16((M, D), 1.0, 781).to(cuda), tr.sprev_vector(D).to(cuda)
        ref, bound = tr.scale_residual_ref(x, y, s)
        xg, yg, sg = f32(x, cuda), b16(y, cuda), f32(s, cuda)
        out = torch.full_like(xg, NAN)
        ext.scale_residual_out(xg, yg, sg, out)
        assert_within(out, ref, bound, f"scale_residual_out {tag}")
        assert torch.equal(xg, f32(x, cuda)), "scale_residual_out changed x"
        ext.scale_residual_(xg, yg, sg)
        assert_within(xg, ref, bound, f"scale_residual_ {tag}")
        g = tr.randn_f32((M, D), 2.0, 782).to(cuda)
        gg = f32(g, cuda)
        q = tr.scale_residual_bwd_ref(g, y, s)
        (ptr,) = poison(cuda, M * D * 2)
        dy, dscale, gsum = ext.scale_residual_bwd(gg, yg, sg)
        landed(dy, ptr, "scale_residual_bwd dy")
        assert_within(dy, q["dy"], q["b_dy"], f"scale_residual_bwd dy {tag}")
        assert_within(dscale, q["dscale"], q["b_dscale"], f"scale_residual_bwd dscale {tag}")
        assert_within(gsum, q["gsum"], q["b_gsum"], f"scale_residual_bwd gsum {tag}")
        gs0, gb0 = f32(tr.randn_f32((D,), 3.0, 783), cuda), f32(tr.randn_f32((D,), 3.0, 784), cuda)
        gs, gb = gs0.clone(), gb0.clone()
        dy2, n1, n2 = ext.scale_residual_bwd(gg, yg, sg, gs, gb)
        assert n1 is None and n2 is None and torch.equal(dy, dy2), f"not deterministic {tag}"
        sink_check(gs, gs0, q["dscale"], q["b_dscale"], f"scale_residual_bwd dscale sink {tag}")
        sink_check(gb, gb0, s * q["gsum"], s.abs() * q["b_gsum"] + tr.U * (s * q["gsum"]).abs(), f"scale_residual_bwd gbias sink {tag}")
        gs2 = gs0.clone()
        ext.scale_residual_bwd(gg, yg, sg, gs2)   # a scale sink alone
        assert torch.equal(gs, gs2), f"dscale sink not deterministic {tag}"


def test_scale_residual_rejects(cuda, ext):
    for D in (12, 2056):
        x, y, s = (torch.zeros(4, D, device=cuda), torch.zeros(4, D, device=cuda, dtype=torch.bfloat16), torch.zeros(D, device=cuda))
        with pytest.raises(RuntimeError):
            ext.scale_residual_bwd(x, y, s)
    with pytest.raises(RuntimeError):
        ext.scale_residual_(torch.zeros(4, 12, device=cuda), torch.zeros(4, 12, device=cuda, dtype=torch.bfloat16),
                            torch.zeros(12, device=cuda))
    x, y, s = (torch.zeros(4, 16, device=cuda), torch.zeros(4, 16, device=cuda, dtype=torch.bfloat16), torch.zeros(16, device=cuda))
    with pytest.raises(RuntimeError, match="bias sink needs a scale sink"):
        ext.scale_residual_bwd(x, y, s, None, torch.zeros(16, device=cuda))


# ---------------------------------------------------------------------------------------------------------------
# cross entropy
XENT_V = [8, 520, 8192, 516, 8196, 32512, 32768, 7, 1001, 1063, 32772, 34999, 35000]   # forms 2, 1, 0


def xent_rows(V):
    rs = [19]
    if tr.xent_form(V) == 0:
        rs += [1, 16, 17, 33]   # across the LDS form's 16-row workgroup
    return rs + {520: [1027], 516: [515]}.get(V, [])   # past the register forms' 1024 / 512 block caps


@pytest.mark.parametrize("V", XENT_V)
def test_xent(cuda, ext, V):
    """xent_fwd_bwd_ and xent_colsum_ (the form V selects): per-row loss, every dlogit, the bias-gradient increments
    against the float64 column sums of the stored dlogits; padding columns exactly zero; two runs bitwise equal."""
    for R in xent_rows(V):
        nrot = 3 if R != 19 else min(12, max(3, max(len(tr.xent_label_kinds(V, r)) for r in range(R))))
        for rot in range(nrot):
            gs = float(torch.tensor(tr.XENT_GSCALES[rot % 3], dtype=torch.float32))
            tag = f"[V {V} R {R} rot {rot} gscale {gs:.3g}]"
            lg, lab = tr.xent_inputs(R, V, rot)
            assert 0 <= int(lab.min()) and int(lab.max()) < V
            lg, lab = lg.to(cuda), lab.to(cuda)
            q = tr.xent_ref(lg, lab, gs)
            zf = b16(lg, cuda)
            loss = ext.xent_fwd_bwd_(zf, lab, gs)
            assert_within(loss, q["loss"], q["b_loss"], f"xent_fwd_bwd_ loss {tag}")
            assert_within(zf, q["dlogits"], q["b_dlogits"], f"xent_fwd_bwd_ dlogits {tag}")
            zf2 = b16(lg, cuda)
            assert torch.equal(ext.xent_fwd_bwd_(zf2, lab, gs), loss) and torch.equal(zf2, zf), f"xent_fwd_bwd_ not deterministic {tag}"
            db0 = f32(tr.randn_f32((V,), 0.01, 790), cuda)
            outs = []
            for _ in range(2):
                z, db = b16(lg, cuda), db0.clone()
                loss = ext.xent_colsum_(z, lab, gs, db)
                outs.append((loss, z, db))
            assert all(torch.equal(a, c) for a, c in zip(*outs)), f"xent_colsum_ not deterministic {tag}"
            assert_within(loss, q["loss"], q["b_loss"], f"xent_colsum_ loss {tag}")
            assert_within(z, q["dlogits"], q["b_dlogits"], f"xent_colsum_ dlogits {tag}")
            s, sb = tr.column_sum_check(z)
            sink_check(db, db0, s, sb, f"xent_colsum_ db {tag}")
            sink_check(db, db0, q["db"], q["b_dlogits"].sum(0) + sb, f"xent_colsum_ db against the reference {tag}")
            if V == tr.XENT_PAD_V:
                for name, zz in (("xent_fwd_bwd_", zf), ("xent_colsum_", z)):
                    assert (zz[:, tr.XENT_PAD_FROM:] == 0).all(), f"{name}: padding dlogits not exactly zero {tag}"
                assert torch.equal(db[tr.XENT_PAD_FROM:], db0[tr.XENT_PAD_FROM:]), f"padding bias increments not zero {tag}"


def test_xent_colsum_rejects_too_wide(cuda, ext):
    z = torch.zeros(2, 35001, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="too wide"):
        ext.xent_colsum_(z, torch.zeros(2, device=cuda, dtype=torch.long), 1.0, torch.zeros(35001, device=cuda))


# ---------------------------------------------------------------------------------------------------------------
# embedding
EMB_V, EMB_VT, EMB_PAD = 3000, 2000, 1900


@pytest.mark.parametrize("d", [4, 256, 2048])
def test_embed_fwd(cuda, ext, d):
    """ids by the BOS / pad / offset rule, rows copied exactly; the flag is 0 on clean input and 1 with an image code
    of V - Vt and a text id of -1, whose ids are clamped; the text-only form with an empty image."""
    table = tr.randn_f32((EMB_V, d), 1.0, 800).to(cuda)
    tg = f32(table, cuda)
    g = torch.Generator().manual_seed(801)
    text = torch.randint(0, EMB_PAD, (3, 6), generator=g)
    text[:, 4:] = 0
    text[1, 0] = 0
    image = torch.randint(0, EMB_V - EMB_VT, (3, 5), generator=g)
    bad_text, bad_image = text.clone(), image.clone()
    bad_text[2, 1] = -1
    bad_image[0, 2] = EMB_V - EMB_VT
    for t, im, flag in ((text, image, 0), (bad_text, bad_image, 1), (text, image[:, :0], 0), (bad_text, image[:, :0], 1)):
        ids, bad = tr.embed_ids_ref(t, im, EMB_PAD, EMB_VT, EMB_V)
        assert bad == flag
        out, ids_k, bad_k = ext.embed_fwd(t.to(cuda), im.to(cuda).contiguous(), tg, EMB_PAD, EMB_VT)
        assert int(bad_k.item()) == flag, "embed_fwd: wrong out-of-table flag"
        assert torch.equal(ids_k.cpu().long(), ids.flatten()), "embed_fwd: wrong ids"
        assert out.shape == (3, ids.shape[1], d) and torch.equal(out, tg[ids.to(cuda)]), "embed_fwd: rows are not exact copies"


@pytest.mark.parametrize("d", [4, 256, 2048])
def test_embed_bwd(cuda, ext, d):
    """Runs of exactly 1, 63, 64, 65, 128, 129 and 500 equal ids into a pre-filled gradient; rows nobody gathered keep
    their content exactly; two runs bitwise equal."""
    ids = tr.embed_run_ids(EMB_V).to(cuda)
    dout = tr.randn_f32((ids.numel(), d), 1.0, 810).to(cuda)
    before = tr.randn_f32((EMB_V, d), 1.0, 811).to(cuda)
    ref, bound = tr.embed_bwd_ref(dout, ids, EMB_V, before)
    order, sorted_ids, head = tr.sort_tables(ids)
    grads = []
    for _ in range(2):
        grad = f32(before, cuda)
        ext.embed_bwd_(f32(dout, cuda), order, sorted_ids, head, grad)
        grads.append(grad)
    assert torch.equal(*grads), "embed_bwd_ not deterministic"
    assert_within(grads[0], ref, bound, f"embed_bwd_ [d {d}]")
    untouched = torch.ones(EMB_V, dtype=torch.bool, device=cuda)
    untouched[ids] = False
    assert torch.equal(grads[0][untouched], f32(before, cuda)[untouched])
