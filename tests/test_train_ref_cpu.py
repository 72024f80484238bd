"""Pins ``tests/train_ref.py`` (the float64 references, inputs and bounds of ``test_train_kernels_gpu.py``) without a
GPU: the references against ``dalle_amd.ops.reference`` + float64 autograd and a brute-force shift map; the measured
constants against a fresh measurement; a dry run of every bound against an fp32 emulation of each kernel (fp32 torch
ops, one rounding to bf16 where the kernel rounds: a bound tighter than correct arithmetic fails here); and the
sensitivity of the bounds: each planted defect, applied to the emulation, exceeds its bound by >= 10 x on an element.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_ref as ar
import train_ref as tr
from dalle_amd.ops import reference as R

f64 = torch.float64


def worst(got, ref, bound):
    """max err / bound over all elements (a bound of 0 demands equality)."""
    err = (got.double() - ref).abs()
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


def close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


# ---------------------------------------------------------------------------------------------------------------
# the reference against torch
PIN_GEOMS = [(1, 8, 64, True), (9, 8, 9, True), (9, 8, 72, True), (9, 8, 73, True), (5, 8, 16, True), (65, 16, 320, True),
             (0, 1, 40, False)]   # T = 1, n = T, n = T + S*S - 1, n = T + S*S, ragged n = T + S + 3


@pytest.mark.parametrize("T,S,n,shift", PIN_GEOMS)
def test_shift_map_is_the_brute_force_loop(T, S, n, shift):
    D = 16
    smap = tr.shift_map(T, S, n, shift)
    y = torch.arange(1, n * D + 1, dtype=f64).view(1, n, D)
    out = tr.apply_shift(y, smap)
    for p in range(n):
        for c in range(D):
            src = p
            if shift and c < D // 2:
                if p < T:
                    src = p - 1 if p >= 1 else -1
                else:
                    r, col = divmod(p - T, S)
                    src = (p - S if r >= 1 else -1) if c < D // 4 else (p - 1 if col >= 1 else -1)
            assert int(smap[p, int(tr.channel_groups(D)[c])]) == src
            assert float(out[0, p, c]) == (float(y[0, src, c]) if src >= 0 else 0.0)
    # unshift is the transpose
    a, b = torch.randn(2, n, D, dtype=f64), torch.randn(2, n, D, dtype=f64)
    close((tr.apply_shift(a, smap) * b).sum(), (a * tr.unshift(b, smap)).sum())


@pytest.mark.parametrize("T,S,n,shift", PIN_GEOMS)
def test_ln_shift_matches_reference_and_autograd(T, S, n, shift):
    B, D = 2, 32
    x = tr.ln_rows("random", B, n, D, seed=1).requires_grad_()
    w, b = (t.requires_grad_() for t in tr.ln_params(D, 1))
    dy = tr.randn_bf16((B, n, D), 1.0, 3)
    resid = tr.randn_f32((B, n, D), 1.0, 4)
    y = R.layernorm_shift(x, w, b, T, S, shift=shift, eps=tr.EPS)
    r = tr.ln_shift_ref(x.detach(), w.detach(), b.detach(), T, S, n, shift)
    close(r["y"], y.detach())
    close(r["mean"], x.detach().mean(-1).reshape(-1))
    close(r["rstd"], (x.detach().var(-1, unbiased=False) + tr.EPS).rsqrt().reshape(-1))
    gx, gw, gb = torch.autograd.grad((y * dy).sum(), (x, w, b))
    for res in (None, resid):
        q = tr.ln_shift_bwd_ref(x.detach(), w.detach(), dy, r["mean"], r["rstd"], r["map"], resid=res)
        close(q["dx"], gx if res is None else gx + res)
        close(q["dw"], gw)
        close(q["db"], gb)


def test_boundary_matches_autograd():
    T, S, n, B, D = 9, 8, 72, 2, 32
    res = tr.ln_rows("random", B, n, D, seed=2)
    yprev = tr.randn_bf16((B, n, D), 1.0, 5).requires_grad_()
    pbias = torch.zeros(D, dtype=f64, requires_grad=True)   # bias of the GEMM whose output was yprev
    sprev = tr.sprev_vector(D).requires_grad_()
    w, b = tr.ln_params(D, 2)
    dy, resid = tr.randn_bf16((B, n, D), 1.0, 6), tr.randn_f32((B, n, D), 1.0, 7)
    x = res + sprev * (yprev + pbias)
    y = R.layernorm_shift(x, w, b, T, S, eps=tr.EPS)
    r = tr.boundary_fwd_ref(res, yprev.detach(), sprev.detach(), w, b, T, S, n, True)
    close(r["xout"], x.detach())
    close(r["y"], y.detach())
    gy, gs, gb = torch.autograd.grad((y * dy).sum() + (x * resid).sum(), (yprev, sprev, pbias))
    q = tr.ln_shift_bwd_ref(x.detach(), w, dy, r["mean"], r["rstd"], r["map"], resid=resid, yprev=yprev.detach(),
                            sprev=sprev.detach())
    close(q["dyprev"], gy)
    close(q["dscale_prev"], gs)
    close(q["dbias_prev"], gb)


def test_geglu_scale_residual_xent_embedding_match_torch():
    h16, h, d = tr.geglu_inputs(7, 24)
    hh = h.clone().requires_grad_()
    out = R.geglu(hh)
    close(tr.geglu_fwd_ref(h)[0], out.detach())
    close(tr.geglu_bwd_ref(h, d)[0], torch.autograd.grad((out * d).sum(), hh)[0])
    assert h16[0, 24].item() == 0 and h16[0, 25].item() == 0 and math.copysign(1, h16[0, 25].item()) == -1
    assert float(h[:, 24:].min()) <= -13.9 and float(h[:, 24:].max()) >= 13.9

    x, y, s = tr.randn_f32((5, 16), 1.0, 1), tr.randn_bf16((5, 16), 1.0, 2).requires_grad_(), tr.sprev_vector(16).requires_grad_()
    g = tr.randn_f32((5, 16), 1.0, 3)
    o = x + s * y
    close(tr.scale_residual_ref(x, y.detach(), s.detach())[0], o.detach())
    gy, gs = torch.autograd.grad((o * g).sum(), (y, s))
    q = tr.scale_residual_bwd_ref(g, y.detach(), s.detach())
    close(q["dy"], gy)
    close(q["dscale"], gs)
    close(q["gsum"], g.sum(0))

    for V in (7, 520, 32512):
        lg, lab = tr.xent_inputs(6, V)
        z = lg.clone().requires_grad_()
        loss = F.cross_entropy(z, lab, reduction="none")
        q = tr.xent_ref(lg, lab, 0.25)
        close(q["loss"], loss.detach(), 1e-11)
        close(q["dlogits"], torch.autograd.grad(loss.sum() * 0.25, z)[0], 1e-11)
        close(q["db"], q["dlogits"].sum(0))
    close(q["loss"][(0 + 0) % 6 + 3], torch.tensor(math.log(tr.XENT_PAD_FROM), dtype=f64), 1e-9)   # the all-equal row
    assert (q["dlogits"][:, tr.XENT_PAD_FROM:] == 0).all()

    V, d_ = 50, 8
    table = tr.randn_f32((V, d_), 1.0, 9).requires_grad_()
    text = torch.tensor([[3, 0, 7, 0], [0, 5, 5, -1]])
    image = torch.tensor([[1, 2, 20], [0, 19, 3]])
    ids, bad = tr.embed_ids_ref(text, image, pad_base=26, Vt=30, V=V)
    assert bad == 1 and ids.tolist() == [[0, 3, 27, 7, 29, 31, 32], [0, 26, 5, 5, 0, 30, 49]]
    assert tr.embed_ids_ref(text.clamp(min=0), image.clamp(max=19), 26, 30, V)[1] == 0
    assert tr.embed_ids_ref(text[:, :2], image[:, :0], 26, 30, V)[0].tolist() == [[0, 3, 27], [0, 26, 5]]
    dout = tr.randn_f32((14, d_), 1.0, 10)
    (gt,) = torch.autograd.grad((table[ids.flatten()] * dout).sum(), table)
    before = tr.randn_f32((V, d_), 1.0, 11)
    close(tr.embed_bwd_ref(dout, ids.flatten(), V, before)[0], before + gt)
    runs = tr.embed_run_ids(3000)
    assert sorted(torch.unique(runs, return_counts=True)[1].tolist()) == [1, 63, 64, 65, 128, 129, 500]


def test_measured_constants_are_what_the_table_says():
    """Each is 4 x a CPU measurement (the formula in fp32 against float64), never a kernel's output."""
    for name, m in (("C_RSQRT", tr.measure_rsqrt_constant()), ("C_ERF", tr.measure_erff_constant()),
                    ("C_AS_EVAL", tr.measure_as_constants()[1])):
        pinned = getattr(tr, name + "_MEASURED")
        assert 0.5 * pinned <= m <= pinned * 1.001, (name, m)
        assert getattr(tr, name) == 4 * pinned
    assert 0.8 * tr.C_AS_FORMULA <= tr.measure_as_constants()[0] <= tr.C_AS_FORMULA
    assert tr.C_T == 4 * ar.C_T_MEASURED and (tr.U, tr.BF, tr.TINY) == (2.0 ** -24, 2.0 ** -8, 2.0 ** -126)


def test_xent_cases_select_the_forms_they_claim():
    """the V list of test_train_kernels_gpu.py: register forms 2 and 1, and the LDS-accumulator form 0; the label
    columns planted for a row lie inside the row and include both ends and the edges of the row's unaligned head."""
    Vs = [8, 520, 8192, 516, 8196, 32512, 32768, 7, 1001, 1063, 32772, 34999, 35000]
    assert [tr.xent_form(V) for V in Vs] == [2, 2, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    assert tr.xent_label_kinds(1001, 1) == [0, 1000, 6, 7, 998, 999]      # head 7, 124 vectors, tail 999, 1000
    assert tr.xent_label_kinds(520, 0) == [0, 519, 8, 15, 511, 512]
    assert max(tr.xent_label_kinds(tr.XENT_PAD_V, 3)) == tr.XENT_PAD_FROM - 1
    for V in Vs:
        for r in range(33):
            assert all(0 <= c < V for c in tr.xent_label_kinds(V, r))


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels (with optional planted defects)
def bf(x):
    return x.to(torch.bfloat16).float()


def emu_ln_fwd(x, w, b, smap, defect=None, res=None):
    """-> mean, rstd, y (bf16 values) [, xout] in fp32. ``res`` = (yprev, sprev): x is the boundary's residual."""
    x, w, b = x.float(), w.float(), b.float()
    if res is not None:
        x = x + res[1].float() * res[0].float()
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    if defect == "one_pass":
        var = (x * x).mean(-1, keepdim=True) - mean * mean
    else:
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
    if defect == "unbiased":
        var = var * (D / (D - 1.0))
    rstd = 1.0 / (var.clamp_min(0).sqrt() + tr.EPS) if defect == "eps_outside" else torch.rsqrt(var + tr.EPS)
    yn = bf((x - mean) * rstd * w + b)
    return mean.reshape(-1), rstd.reshape(-1), tr.apply_shift(yn, smap), x


def emu_ln_bwd(x, w, dy, mean, rstd, smap, resid=None, yprev=None, sprev=None, defect=None):
    B, n, D = x.shape
    x, w, m, r = x.float(), w.float(), mean.float().view(B, n, 1), rstd.float().view(B, n, 1)
    g = tr.unshift(dy.float(), smap)
    xh = (x - m) * r
    gy = g * w
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    dx = r * (gy - s1 - xh * s2)
    if resid is not None:
        dx = resid.float() + dx
    keep = slice(4, None) if defect == "missing_partial" else slice(None)   # one workgroup's four rows
    out = {"dx": dx, "dw": (g * xh).flatten(0, 1)[keep].sum(0), "db": g.flatten(0, 1)[keep].sum(0)}
    if yprev is not None:
        s = sprev.float()
        out.update(dyprev=bf(s * dx), dscale_prev=(dx * yprev.float()).sum((0, 1)),
                   dbias_prev=dx.sum((0, 1)) * (1.0 if defect == "no_sprev" else s))
    return out


def emu_geglu_fwd(h, defect=None):
    a, g = h.float().chunk(2, dim=-1)
    if defect == "tanh":
        return bf(a * F.gelu(g, approximate="tanh"))
    return bf(a * (0.5 * g * (1.0 + torch.erf(g * torch.tensor(tr.SQRT1_2, dtype=torch.float32)))))


def emu_geglu_bwd(h, d):
    a, g = h.float().chunk(2, dim=-1)
    erf_abs, e = tr.as_erf_abs(g.abs() * torch.tensor(tr.SQRT1_2, dtype=torch.float32), g)
    cdf = 0.5 + 0.5 * torch.copysign(erf_abs, g)
    ge, gr = g * cdf, g * torch.tensor(tr.INV_SQRT_2PI, dtype=torch.float32) * e + cdf
    return torch.cat([bf(d.float() * ge), bf(d.float() * a * gr)], dim=-1)


def emu_xent(logits, labels, gscale, defect=None):
    """-> loss, dlogits (bf16 values), db in fp32: exp as exp2 of the product with log2e, as ``__expf`` is."""
    f = logits.float()
    l2e = torch.tensor(tr.LOG2E, dtype=torch.float32)
    m = f.max(-1, keepdim=True).values
    s = torch.exp2((f - m) * l2e).sum(-1, keepdim=True)
    lse = m + torch.log2(s) * torch.tensor(math.log(2.0), dtype=torch.float32)
    p = torch.exp2((f - lse) * l2e)
    lab = (labels + 1) % f.shape[1] if defect == "label_off" else labels
    g32 = (p - torch.zeros_like(p).scatter_(1, lab.view(-1, 1), 1.0)) * torch.tensor(gscale, dtype=torch.float32)
    g = bf(g32)
    db = (g32 if defect == "db_fp32" else g).sum(0)
    return (lse - f.gather(1, labels.view(-1, 1))).squeeze(-1), g, db


# ---------------------------------------------------------------------------------------------------------------
# dry run: correct fp32 arithmetic passes every bound
DRY_LN = [(256, 9, 8, 72, True), (2048, 5, 8, 16, True), (512, 65, 16, 320, True), (1024, 0, 1, 40, False), (256, 1, 8, 1, True)]


def _ln_case(D, T, S, n, shift, kind, B=3):
    B = 1 if n == 1 else B
    x = tr.ln_rows(kind, B, n, D)
    w, b = tr.ln_params(D)
    return B, x, w, b


@pytest.mark.parametrize("kind", tr.LN_KINDS)
@pytest.mark.parametrize("D,T,S,n,shift", DRY_LN)
def test_dry_run_layernorm(D, T, S, n, shift, kind):
    B, x, w, b = _ln_case(D, T, S, n, shift, kind)
    r = tr.ln_shift_ref(x, w, b, T, S, n, shift)
    mean, rstd, y, _ = emu_ln_fwd(x, w, b, r["map"])
    for name, got in (("mean", mean), ("rstd", rstd), ("y", y)):
        assert worst(got, r[name], r["b_" + name]) <= 1.0, (name, worst(got, r[name], r["b_" + name]))
    dy, resid = tr.randn_bf16((B, n, D), 1.0, 11), tr.randn_f32((B, n, D), 1.0, 12)
    m32, r32 = tr.f32_round(r["mean"]), tr.f32_round(r["rstd"])
    for res in (None, resid):
        q = tr.ln_shift_bwd_ref(x, w, dy, m32, r32, r["map"], resid=res)
        e = emu_ln_bwd(x, w, dy, m32, r32, r["map"], resid=res)
        for name in ("dx", "dw", "db"):
            assert worst(e[name], q[name], q["b_" + name]) <= 1.0, (name, worst(e[name], q[name], q["b_" + name]))


@pytest.mark.parametrize("kind", tr.LN_KINDS)
@pytest.mark.parametrize("D,T,S,n", [(256, 9, 8, 72), (2048, 9, 8, 72)])
def test_dry_run_boundary(D, T, S, n, kind):
    B = 2
    res, (w, b) = tr.ln_rows(kind, B, n, D), tr.ln_params(D)
    yprev, sprev = tr.randn_bf16((B, n, D), 1.0, 13), tr.sprev_vector(D)
    r = tr.boundary_fwd_ref(res, yprev, sprev, w, b, T, S, n, True)
    mean, rstd, y, xout = emu_ln_fwd(res, w, b, r["map"], res=(yprev, sprev))
    for name, got in (("mean", mean), ("rstd", rstd), ("y", y), ("xout", xout)):
        assert worst(got, r[name], r["b_" + name]) <= 1.0, (name, worst(got, r[name], r["b_" + name]))
    x = tr.f32_round(r["xout"])
    dy, resid = tr.randn_bf16((B, n, D), 1.0, 14), tr.randn_f32((B, n, D), 1.0, 15)
    m32, r32 = tr.f32_round(r["mean"]), tr.f32_round(r["rstd"])
    q = tr.ln_shift_bwd_ref(x, w, dy, m32, r32, r["map"], resid=resid, yprev=yprev, sprev=sprev)
    e = emu_ln_bwd(x, w, dy, m32, r32, r["map"], resid=resid, yprev=yprev, sprev=sprev)
    for name in ("dx", "dw", "db", "dyprev", "dscale_prev", "dbias_prev"):
        assert worst(e[name], q[name], q["b_" + name]) <= 1.0, (name, worst(e[name], q[name], q["b_" + name]))


@pytest.mark.parametrize("M,F", [(1, 8), (300, 512), (64, 2056)])
def test_dry_run_geglu(M, F):
    h16, h, d = tr.geglu_inputs(M, F)
    ref, bound = tr.geglu_fwd_ref(h)
    assert worst(emu_geglu_fwd(h16), ref, bound) <= 1.0, worst(emu_geglu_fwd(h16), ref, bound)
    ref, bound = tr.geglu_bwd_ref(h, d)
    dh = emu_geglu_bwd(h16, d)
    assert worst(dh, ref, bound) <= 1.0, worst(dh, ref, bound)
    s, b = tr.column_sum_check(dh)
    assert worst(dh.sum(0), s, b) <= 1.0


@pytest.mark.parametrize("V", [7, 520, 516, 1063, 32512, 35000])
def test_dry_run_xent(V):
    for rot, gs in enumerate(tr.XENT_GSCALES):
        gs = float(torch.tensor(gs, dtype=torch.float32))
        lg, lab = tr.xent_inputs(7, V, rot)
        q = tr.xent_ref(lg, lab, gs)
        loss, g, db = emu_xent(lg, lab, gs)
        assert worst(loss, q["loss"], q["b_loss"]) <= 1.0, worst(loss, q["loss"], q["b_loss"])
        assert worst(g, q["dlogits"], q["b_dlogits"]) <= 1.0, worst(g, q["dlogits"], q["b_dlogits"])
        s, b = tr.column_sum_check(g)
        assert worst(db, s, b) <= 1.0
        if V == tr.XENT_PAD_V:
            assert (g[:, tr.XENT_PAD_FROM:] == 0).all() and (db[tr.XENT_PAD_FROM:] == 0).all()


def test_dry_run_scale_residual_and_embedding():
    M, D = 77, 776
    x, y, s, g = tr.randn_f32((M, D), 1.0, 1), tr.randn_bf16((M, D), 1.0, 2), tr.sprev_vector(D), tr.randn_f32((M, D), 1.0, 3)
    ref, bound = tr.scale_residual_ref(x, y, s)
    assert worst(x.float() + s.float() * y.float(), ref, bound) <= 1.0
    q = tr.scale_residual_bwd_ref(g, y, s)
    assert worst(bf(g.float() * s.float()), q["dy"], q["b_dy"]) <= 1.0
    assert worst((g.float() * y.float()).sum(0), q["dscale"], q["b_dscale"]) <= 1.0
    assert worst(g.float().sum(0), q["gsum"], q["b_gsum"]) <= 1.0
    ids = tr.embed_run_ids(3000)
    dout, before = tr.randn_f32((ids.numel(), 8), 1.0, 4), tr.randn_f32((3000, 8), 1.0, 5)
    ref, bound = tr.embed_bwd_ref(dout, ids, 3000, before)
    assert worst(before.float().index_add(0, ids, dout.float()), ref, bound) <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# sensitivity: each planted defect is >= 10 x outside a bound on some element
def _ratio_ln_fwd(kind, defect=None, mapfix=None, D=256, geom=(9, 8, 72, True)):
    T, S, n, shift = geom
    B, x, w, b = _ln_case(D, T, S, n, shift, kind)
    r = tr.ln_shift_ref(x, w, b, T, S, n, shift)
    smap = r["map"].clone()
    if mapfix:
        mapfix(smap, T, S)
    mean, rstd, y, _ = emu_ln_fwd(x, w, b, smap, defect)
    return max(worst(rstd, r["rstd"], r["b_rstd"]), worst(y, r["y"], r["b_y"]))


@pytest.mark.parametrize("defect,kind", [("one_pass", "offset"), ("unbiased", "random"), ("eps_outside", "scaled"),
                                         ("eps_outside", "constant")])
def test_variance_defects_are_caught(defect, kind):
    assert _ratio_ln_fwd(kind) <= 1.0
    ratio = _ratio_ln_fwd(kind, defect)
    print(defect, kind, ratio)
    assert ratio >= 10.0, ratio


def _set(p, groups, src):
    def fix(smap, T, S):
        pos, s = p(T, S), src(T, S)
        for gi in groups:
            smap[pos, gi] = s
    return fix


MAP_DEFECTS = {
    "first_image_row_takes_a_row_above": _set(lambda T, S: T + 2, (0,), lambda T, S: T + 2 - S),
    "first_column_takes_the_previous_rows_end": _set(lambda T, S: T + 2 * S, (1,), lambda T, S: T + 2 * S - 1),
    "image_above_off_by_one_column": _set(lambda T, S: T + 2 * S + 3, (0,), lambda T, S: T + S + 2),
    "image_left_off_by_one_row": _set(lambda T, S: T + 2 * S + 3, (1,), lambda T, S: T + S + 2),
    "last_text_position_off_by_one": _set(lambda T, S: T - 1, (0, 1), lambda T, S: T - 3),
    "position_0_takes_position_1": _set(lambda T, S: 0, (0, 1), lambda T, S: 1),
    "owed_zero_left_unshifted_at_0": _set(lambda T, S: 0, (0, 1), lambda T, S: 0),
    "owed_zero_left_unshifted_first_image": _set(lambda T, S: T, (0, 1), lambda T, S: T),
    "text_shifts_one_quarter": _set(lambda T, S: slice(1, T), (1,), lambda T, S: torch.arange(1, T)),
}


@pytest.mark.parametrize("name", sorted(MAP_DEFECTS))
def test_shift_defects_are_caught(name):
    ratio = _ratio_ln_fwd("random", mapfix=MAP_DEFECTS[name])
    print(name, ratio)
    assert ratio >= 10.0, ratio


def test_gelu_label_and_column_sum_defects_are_caught():
    h16, h, d = tr.geglu_inputs(64, 512)
    ref, bound = tr.geglu_fwd_ref(h)
    ratio = worst(emu_geglu_fwd(h16, "tanh"), ref, bound)
    print("tanh-GELU", ratio)
    assert ratio >= 10.0, ratio

    for gs in tr.XENT_GSCALES:
        gs = float(torch.tensor(gs, dtype=torch.float32))
        lg, lab = tr.xent_inputs(19, 1001)
        q = tr.xent_ref(lg, lab, gs)
        _, g, _ = emu_xent(lg, lab, gs, "label_off")
        assert worst(g, q["dlogits"], q["b_dlogits"]) >= 10.0
        # the bias gradient sums the stored bf16 values, not the fp32 values before rounding: distinguishable
        _, g, db = emu_xent(lg, lab, gs, "db_fp32")
        s, b = tr.column_sum_check(g)
        ratio = worst(db, s, b)
        print("db from fp32 dlogits, gscale", gs, ratio)
        assert ratio >= 10.0, ratio

    D, T, S, n, B = 256, 9, 8, 72, 2
    x, (w, b) = tr.ln_rows("random", B, n, D), tr.ln_params(D)
    yprev, sprev = tr.randn_bf16((B, n, D), 1.0, 13), tr.sprev_vector(D)
    dy, resid = tr.randn_bf16((B, n, D), 1.0, 14), tr.randn_f32((B, n, D), 1.0, 15)
    r = tr.ln_shift_ref(x, w, b, T, S, n, True)
    m32, r32 = tr.f32_round(r["mean"]), tr.f32_round(r["rstd"])
    q = tr.ln_shift_bwd_ref(x, w, dy, m32, r32, r["map"], resid=resid, yprev=yprev, sprev=sprev)
    e = emu_ln_bwd(x, w, dy, m32, r32, r["map"], resid=resid, yprev=yprev, sprev=sprev, defect="no_sprev")
    assert worst(e["dbias_prev"], q["dbias_prev"], q["b_dbias_prev"]) >= 10.0
    e = emu_ln_bwd(x, w, dy, m32, r32, r["map"], resid=resid, defect="missing_partial")
    for name in ("dw", "db"):
        ratio = worst(e[name], q[name], q["b_" + name])
        print("missing partial row", name, ratio)
        assert ratio >= 10.0, ratio
