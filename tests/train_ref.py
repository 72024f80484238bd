"""Float64 references of the residual-stream training kernels (K1-K4 LayerNorm + token shift and its fused sublayer
boundary, K8 / K10 LayerScale residual, K9 GEGLU, K12 fused cross entropy, K1 / K2 embedding), the seeded inputs of
``test_train_kernels_gpu.py`` and its per-element bounds. No GPU code and no dependence on the extension: plain torch
in float64, pinned to ``ops.reference`` + autograd and to brute-force loops by ``test_train_ref_cpu.py``. Every
function runs on whatever device its inputs are on.

The references read what the kernels read: bf16 operands as bf16 values upcast, fp32 operands as fp32 values upcast.
The bounds (derived in ``test_train_kernels_gpu.py``'s docstring) are formed from reference quantities only.
"""
from __future__ import annotations

import math

import torch

from attn_ref import BF, C_T, TINY, U, bf16_round  # noqa: F401  (re-exported: one set of constants for both modules)

EPS = 1e-5
SQRT1_2 = 0.70710678118654752
INV_SQRT_2PI = 0.3989422804014327
LOG2E = 1.0 / math.log(2.0)
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def f32_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).double()


# ---------------------------------------------------------------------------------------------------------------
# measured constants (re-measured by test_train_ref_cpu.py; none comes from a kernel's output)
def measure_rsqrt_constant(n: int = 1 << 16, seed: int = 0) -> float:
    """rsqrt evaluated in fp32 on the CPU against float64, for arguments 1e-6 .. 1e9: max relative error."""
    g = torch.Generator().manual_seed(seed)
    v = torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * math.log(1e15) + math.log(1e-6)).float()
    r32, r64 = torch.rsqrt(v).double(), torch.rsqrt(v.double())
    return ((r32 - r64).abs() / r64).max().item()


def measure_erff_constant(n: int = 1 << 16, seed: int = 0) -> float:
    """erff evaluated in fp32 on the CPU against float64 erf for arguments in [-10, 10]: max relative error."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand(n, generator=g, dtype=torch.float64) * 20.0 - 10.0).float()
    z = z[z != 0]
    e32, e64 = torch.erf(z).double(), torch.erf(z.double())
    return ((e32 - e64).abs() / e64.abs()).max().item()


def as_erf_abs(z: torch.Tensor, x: torch.Tensor):
    """``gelu_and_grad``'s erf(|x| / sqrt 2) (Abramowitz-Stegun 7.1.26) and its exp(-x^2 / 2), in z's dtype with the
    kernel's operation order: z = |x| / sqrt 2. Returns (erf_abs, e)."""
    t = 1.0 / (AS_P * z + 1.0)
    poly = t * (t * (t * (t * (t * AS_A[4] + AS_A[3]) + AS_A[2]) + AS_A[1]) + AS_A[0])
    e = torch.exp2(-0.5 * x * x * LOG2E)
    return 1.0 - poly * e, e


def measure_as_constants(n: int = 1 << 16, seed: int = 0):
    """-> (formula, evaluation): the Abramowitz-Stegun formula's own absolute error on erf (float64 evaluation against
    erf; the handbook's 1.5e-7), and the absolute error of evaluating it in fp32 on the CPU (against its float64
    evaluation), for |x| <= 14."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, generator=g, dtype=torch.float64) * 28.0 - 14.0
    x = x.float().double()
    e64, _ = as_erf_abs(x.abs() * SQRT1_2, x)
    x32 = x.float()
    e32, _ = as_erf_abs(x32.abs() * torch.tensor(SQRT1_2, dtype=torch.float32), x32)
    formula = (e64 - torch.erf(x.abs() * SQRT1_2)).abs().max().item()
    return formula, (e32.double() - e64).abs().max().item()


C_RSQRT_MEASURED = 8.81e-8     # measure_rsqrt_constant()
C_RSQRT = 4 * C_RSQRT_MEASURED   # hardware rsqrt
C_ERF_MEASURED = 5.99e-8       # measure_erff_constant()
C_ERF = 4 * C_ERF_MEASURED     # ocml erff
C_AS_FORMULA = 1.5e-7          # Abramowitz-Stegun 7.1.26 (the handbook's figure; measure_as_constants()[0] is below it)
C_AS_EVAL_MEASURED = 3.44e-7   # measure_as_constants()[1]
C_AS_EVAL = 4 * C_AS_EVAL_MEASURED   # the polynomial, rcp and exp2 in fp32 on the hardware


# ---------------------------------------------------------------------------------------------------------------
# token shift
def channel_groups(D: int, device=None) -> torch.Tensor:
    """(D,) 0 for [0, D/4), 1 for [D/4, D/2), 2 for [D/2, D)."""
    c = torch.arange(D, device=device)
    return (c >= D // 4).long() + (c >= D // 2).long()


def shift_map(T: int, S: int, n: int, shift: bool, device=None) -> torch.Tensor:
    """(n, 3) long: the source position that feeds (position, channel group), -1 where zeros are owed. Text positions
    take groups 0 and 1 from the previous position; image position k = p - T takes group 0 from the token above
    (k >= S) and group 1 from the token to the left (k % S != 0); group 2 never moves."""
    p = torch.arange(n, device=device)
    if not shift:
        return torch.stack([p, p, p], dim=1)
    text = p < T
    k = p - T
    neg = torch.full_like(p, -1)
    prev = torch.where(p >= 1, p - 1, neg)
    g0 = torch.where(text, prev, torch.where(k >= S, p - S, neg))
    g1 = torch.where(text, prev, torch.where(k % S != 0, p - 1, neg))
    return torch.stack([g0, g1, p], dim=1)


def apply_shift(y: torch.Tensor, smap: torch.Tensor) -> torch.Tensor:
    """y (B, n, D) -> out[:, p, group cols] = y[:, smap[p, group], group cols], zeros where the map is -1."""
    grp = channel_groups(y.shape[-1], y.device)
    out = torch.zeros_like(y)
    for gi in range(3):
        src = smap[:, gi]
        ok = (src >= 0).nonzero().flatten()
        cols = (grp == gi).nonzero().flatten()
        out[:, ok[:, None], cols[None, :]] = y[:, src[ok][:, None], cols[None, :]]
    return out


def unshift(dy: torch.Tensor, smap: torch.Tensor) -> torch.Tensor:
    """The transpose of ``apply_shift``: g[:, smap[p, group], group cols] = dy[:, p, group cols] (a source feeds at
    most one position per group), zeros for sources nobody reads."""
    grp = channel_groups(dy.shape[-1], dy.device)
    out = torch.zeros_like(dy)
    for gi in range(3):
        src = smap[:, gi]
        ok = (src >= 0).nonzero().flatten()
        cols = (grp == gi).nonzero().flatten()
        out[:, src[ok][:, None], cols[None, :]] = dy[:, ok[:, None], cols[None, :]]
    return out


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm + token shift
def ln_depth(D: int) -> int:
    """additions a term of a row sum passes through: D / 64 per lane in sequence, then the 6-level butterfly."""
    return D // 64 + 6


def ln_shift_ref(x, w, b, T, S, n, shift, eps=EPS, dx_in=None):
    """x (B, n, D) float64, w / b (D,). Returns a dict: ``mean`` / ``rstd`` (B*n,), ``yn`` (the normalised rows),
    ``y`` (after the shift), ``map`` (n, 3), and the bounds ``b_mean``, ``b_rstd``, ``b_y`` (zero where zeros are
    owed). ``dx_in``: per-element error of the x the kernel normalises (the fused boundary forms it in fp32)."""
    B, _, D = x.shape
    dep = ln_depth(D)
    e_x = torch.zeros_like(x) if dx_in is None else dx_in
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    yn = d * rstd * w + b
    smap = shift_map(T, S, n, shift, x.device)
    e_m = dep * U * x.abs().mean(-1, keepdim=True) + U * mean.abs() + e_x.mean(-1, keepdim=True)
    # sum (x - m^)^2 = sum (x - m)^2 + D (m - m^)^2: the mean's own error enters the variance squared
    e_var = (dep + 4) * U * var + e_m * e_m + (2 * d.abs() * e_x + e_x * e_x).mean(-1, keepdim=True)
    b_rstd = rstd * (0.5 * e_var / (var + eps) + C_RSQRT + 2 * U)
    e_d = e_m + e_x + U * d.abs()
    e_yn = w.abs() * (rstd * e_d + d.abs() * b_rstd) + 3 * U * (d * rstd * w).abs() + U * yn.abs()
    b_yn = BF * yn.abs() + (1 + BF) * e_yn + TINY
    return {"mean": mean.reshape(-1), "rstd": rstd.reshape(-1), "yn": yn, "y": apply_shift(yn, smap), "map": smap,
            "b_mean": e_m.reshape(-1), "b_rstd": b_rstd.reshape(-1), "b_y": apply_shift(b_yn, smap)}


def ln_shift_bwd_ref(x, w, dy, mean, rstd, smap, resid=None, yprev=None, sprev=None):
    """x (B, n, D), dy (B, n, D) (bf16 values), mean / rstd (B*n,) as the kernel is given them (fp32 values). Returns
    ``dx`` (with ``resid`` added when given), ``dw``, ``db`` and their bounds; with ``yprev`` / ``sprev`` also the fused
    boundary's ``dyprev = sprev dx``, ``dscale_prev = sum_rows dx yprev``, ``dbias_prev = sprev sum_rows dx``."""
    B, n, D = x.shape
    rows, dep = B * n, ln_depth(D)
    m, r = mean.view(B, n, 1), rstd.view(B, n, 1)
    g = unshift(dy, smap)
    xh = (x - m) * r
    gy = g * w
    s1 = gy.mean(-1, keepdim=True)
    s2 = (gy * xh).mean(-1, keepdim=True)
    core = r * (gy - s1 - xh * s2)
    dx = core if resid is None else resid + core
    e_xh = 3 * U * xh.abs()
    e_s1 = (dep + 1) * U * gy.abs().mean(-1, keepdim=True)
    e_s2 = (dep + 2) * U * (gy * xh).abs().mean(-1, keepdim=True) + (gy.abs() * e_xh).mean(-1, keepdim=True)
    mag = r * (gy.abs() + s1.abs() + (xh * s2).abs())
    e_dx = r * (U * gy.abs() + e_s1 + xh.abs() * e_s2 + e_xh * s2.abs()) + 4 * U * mag + U * dx.abs()
    if resid is not None:
        e_dx = e_dx + U * resid.abs()
    out = {"dx": dx, "b_dx": e_dx + TINY, "dw": (g * xh).sum((0, 1)), "db": g.sum((0, 1)),
           "b_dw": (rows + 1) * U * (g * xh).abs().sum((0, 1)) + (g.abs() * e_xh).sum((0, 1)) + TINY,
           "b_db": rows * U * g.abs().sum((0, 1)) + TINY}
    if yprev is not None:
        dyp = sprev * dx
        out.update(dyprev=dyp, b_dyprev=BF * dyp.abs() + (1 + BF) * (sprev.abs() * e_dx + U * dyp.abs()) + TINY,
                   dscale_prev=(dx * yprev).sum((0, 1)), dbias_prev=sprev * dx.sum((0, 1)),
                   b_dscale_prev=(rows + 1) * U * (dx * yprev).abs().sum((0, 1)) + (e_dx * yprev.abs()).sum((0, 1)) + TINY,
                   b_dbias_prev=sprev.abs() * (rows * U * dx.abs().sum((0, 1)) + e_dx.sum((0, 1)))
                   + U * (sprev * dx.sum((0, 1))).abs() + TINY)
    return out


def boundary_fwd_ref(res, yprev, sprev, w, b, T, S, n, shift, eps=EPS):
    """The fused sublayer boundary: ``xout = res + sprev * yprev`` (one fp32 multiply-add) and its LayerNorm + shift."""
    x = res + sprev * yprev
    b_x = 2 * U * (res.abs() + (sprev * yprev).abs())
    out = ln_shift_ref(x, w, b, T, S, n, shift, eps, dx_in=b_x)
    out.update(xout=x, b_xout=b_x)
    return out


def sink_slack(before, ref):
    """the fp32 add of a computed value into a sink's prior content."""
    return 2 * U * (before.abs() + ref.abs())


# ---------------------------------------------------------------------------------------------------------------
# GEGLU
def gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g * SQRT1_2))


def gelu_grad64(g):
    return 0.5 * (1.0 + torch.erf(g * SQRT1_2)) + g * INV_SQRT_2PI * torch.exp(-0.5 * g * g)


def geglu_fwd_ref(h):
    """h (M, 2F) bf16 values -> out = a * gelu(g) with the exact erf, and its bound."""
    a, g = h.chunk(2, dim=-1)
    erf = torch.erf(g * SQRT1_2)
    out = a * gelu64(g)
    # erf'(z) dz of the rounded argument g / sqrt 2 (the constant's and the product's rounding), ocml erff, 1 + erf
    e_erf = 2.0 / math.sqrt(math.pi) * torch.exp(-0.5 * g * g) * 2 * U * (g * SQRT1_2).abs() + C_ERF * erf.abs() + U * (1 + erf.abs())
    e_gelu = 0.5 * g.abs() * e_erf + 2 * U * gelu64(g).abs()
    return out, BF * out.abs() + (1 + BF) * (a.abs() * e_gelu + U * out.abs()) + TINY


def geglu_bwd_ref(h, d):
    """h (M, 2F), d (M, F) -> dh = [d gelu(g) | d a gelu'(g)] and its bound (``gelu_and_grad``'s approximation)."""
    a, g = h.chunk(2, dim=-1)
    ge, gr = gelu64(g), gelu_grad64(g)
    da, dg = d * ge, d * a * gr
    e_cdf = 0.5 * (C_AS_FORMULA + C_AS_EVAL) + U + TINY
    e_ge = g.abs() * e_cdf + U * ge.abs()
    pdf = g.abs() * INV_SQRT_2PI * torch.exp(-0.5 * g * g)
    e_gr = e_cdf + pdf * (2 * U * g * g + 2 * U + C_T) + U * gr.abs() + TINY
    b_da = BF * da.abs() + (1 + BF) * (d.abs() * e_ge + U * da.abs()) + TINY
    b_dg = BF * dg.abs() + (1 + BF) * ((d * a).abs() * e_gr + 2 * U * dg.abs()) + TINY
    return torch.cat([da, dg], dim=-1), torch.cat([b_da, b_dg], dim=-1)


def column_sum_check(stored, rows=None):
    """float64 column sums of the values a kernel stored, and the bound of a fixed-order fp32 sum of them."""
    s = stored.double()
    rows = s.shape[0] if rows is None else rows
    return s.sum(0), rows * U * s.abs().sum(0) + TINY


# ---------------------------------------------------------------------------------------------------------------
# LayerScale residual
def scale_residual_ref(x, y, s):
    out = x + s * y
    return out, 2 * U * (x.abs() + (s * y).abs())


def scale_residual_bwd_ref(g, y, s):
    """g (M, D) fp32 values, y bf16 values, s (D,). -> dy = s g, dscale = sum_rows g y, gsum = sum_rows g, bounds."""
    M = g.shape[0]
    dy = s * g
    return {"dy": dy, "b_dy": BF * dy.abs() + (1 + BF) * U * dy.abs() + TINY,
            "dscale": (g * y).sum(0), "b_dscale": (M + 1) * U * (g * y).abs().sum(0) + TINY,
            "gsum": g.sum(0), "b_gsum": M * U * g.abs().sum(0) + TINY}


# ---------------------------------------------------------------------------------------------------------------
# cross entropy
def xent_chain(V: int):
    """-> (K, N_ADD): exp evaluations a term's factor passes through (the online forms rescale the running sum once
    per 8-column step of a thread, then per wave and per workgroup) and additions on its way into the row sum."""
    steps = -(-V // 2048)
    return steps + 3, 8 * steps + 32


def xent_ref(logits, labels, gscale):
    """logits (R, V) bf16 values, labels (R,), gscale as the kernel receives it (fp32 value). -> dict: ``loss``,
    ``dlogits``, ``lse``, ``db`` (column sums of dlogits) and ``b_loss``, ``b_dlogits``."""
    R, V = logits.shape
    K, n_add = xent_chain(V)
    m = logits.max(-1, keepdim=True).values
    xm = logits - m
    ex = torch.exp(xm)
    S = ex.sum(-1, keepdim=True)
    lse = m + torch.log(S)
    p = ex / S
    xl = logits.gather(1, labels.view(-1, 1))
    loss = (lse - xl).squeeze(-1)
    onehot = torch.zeros_like(logits).scatter_(1, labels.view(-1, 1), 1.0)
    G = (p - onehot) * gscale
    # relative error of the row sum: every term exp(f - M) with its exponent's three roundings, K evaluations, the adds
    e_S = (p * 3 * U * xm.abs()).sum(-1, keepdim=True) + K * (3 * U + C_T) + n_add * U
    e_lse = e_S + (C_T + 2 * U) * torch.log2(S).abs().clamp_min(1.0) + U * lse.abs()
    b_loss = (e_lse + U * (lse.abs() + loss.abs().unsqueeze(-1))).squeeze(-1)
    rel_p = 3 * U * (logits - lse).abs() + 2 * U + C_T + e_lse + U * lse.abs()
    b_G = BF * G.abs() + (1 + BF) * (abs(gscale) * p * rel_p + 2 * U * G.abs()) + TINY
    return {"loss": loss, "lse": lse.squeeze(-1), "dlogits": G, "db": G.sum(0), "b_loss": b_loss, "b_dlogits": b_G, "p": p}


# ---------------------------------------------------------------------------------------------------------------
# embedding
def embed_ids_ref(text, image, pad_base, Vt, V):
    """text (B, Ttxt), image (B, Timg) int64 -> (ids (B, n) int64 clamped into the table, flag): position 0 is BOS
    (id 0), positions 1..Ttxt the text ids with 0 replaced by the per-position pad id ``pad_base + p - 1``, the rest
    ``Vt + image code`` with the last image token dropped (n = Ttxt + Timg, or Ttxt + 1 without an image)."""
    B, Ttxt = text.shape
    Timg = image.shape[1]
    pos = torch.arange(Ttxt, device=text.device)
    t = torch.where(text == 0, pad_base + pos, text)
    parts = [torch.zeros(B, 1, dtype=torch.long, device=text.device), t]
    if Timg > 0:
        parts.append(Vt + image[:, :Timg - 1])
    ids = torch.cat(parts, dim=1)
    bad = int(((ids < 0) | (ids >= V)).any())
    return ids.clamp(0, V - 1), bad


def embed_bwd_ref(dout, ids, V, before):
    """dout (N, d), ids (N,) -> before + index_add, and the bound of the fixed-order sums: run length u sum |rows|."""
    N, d = dout.shape
    add = torch.zeros(V, d, dtype=torch.float64, device=dout.device).index_add_(0, ids, dout)
    mag = torch.zeros(V, d, dtype=torch.float64, device=dout.device).index_add_(0, ids, dout.abs())
    run = torch.zeros(V, dtype=torch.float64, device=dout.device).index_add_(0, ids, torch.ones(N, dtype=torch.float64, device=dout.device))
    return before + add, (run.view(-1, 1) + 1) * U * (mag + before.abs()) + TINY


def sort_tables(ids):
    """the stable sort tables ``embed_bwd_`` is given: order, sorted ids, head (first sorted position of the run)."""
    sorted_ids, order = torch.sort(ids, stable=True)
    n = ids.numel()
    pos = torch.arange(n, device=ids.device)
    start = torch.ones(n, dtype=torch.bool, device=ids.device)
    start[1:] = sorted_ids[1:] != sorted_ids[:-1]
    head = torch.cummax(torch.where(start, pos, torch.zeros_like(pos)), 0).values
    return order.to(torch.int32), sorted_ids.to(torch.int32).contiguous(), head.to(torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs
LN_KINDS = ("random", "offset", "constant", "scaled")
LN_GEOMS = [(1, 8, 64, True), (9, 8, 72, True), (65, 16, 320, True), (33, 32, 33, True), (5, 8, 16, True),
            (7, 8, 71, True), (0, 1, 40, False)]   # (T, S, n, shift); the last is the final norm of logits_loss


def ln_rows(kind: str, B: int, n: int, D: int, seed: int = 0) -> torch.Tensor:
    """(B, n, D) fp32-valued float64 rows. random: N(0, 1) scaled per row by 1 + 0.25 (row % 5) (a row read from the
    wrong position is far outside the bounds); offset: even rows 100 + N(0, 1), odd rows -300 + 0.01 N(0, 1) (mean >>
    std: a one-pass variance fails); constant: every third row constant (variance 0, rstd = eps^-1/2), the rest random;
    scaled: row 0 times 1e4 and row 1 (or the last) times 1e-4."""
    g = torch.Generator().manual_seed(100 + seed)
    z = torch.randn(B * n, D, generator=g, dtype=torch.float64)
    r = torch.arange(B * n, dtype=torch.float64).view(-1, 1)
    x = z * (1.0 + 0.25 * (r % 5))
    if kind == "offset":
        x = torch.where(r % 2 == 0, 100.0 + z, -300.0 + 0.01 * z)
    elif kind == "constant":
        c = 0.37 * (r % 7 - 3.0) + 0.011
        x = torch.where(r % 3 == 0, c.expand_as(x), x)
    elif kind == "scaled":
        x[0] *= 1e4
        x[min(1, B * n - 1)] *= 1e-4 if B * n > 1 else 1.0
    elif kind != "random":
        raise ValueError(kind)
    return f32_round(x).view(B, n, D)


def ln_params(D: int, seed: int = 0):
    g = torch.Generator().manual_seed(200 + seed)
    w = f32_round(1.0 + 0.5 * torch.randn(D, generator=g, dtype=torch.float64))
    b = f32_round(0.3 * torch.randn(D, generator=g, dtype=torch.float64))
    return w, b


def randn_bf16(shape, std: float, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return bf16_round(torch.randn(shape, generator=g, dtype=torch.float64) * std)


def randn_f32(shape, std: float, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return f32_round(torch.randn(shape, generator=g, dtype=torch.float64) * std)


def sprev_vector(D: int, seed: int = 0) -> torch.Tensor:
    """LayerScale of the previous sublayer: mixed signs, one exact zero column."""
    s = randn_f32((D,), 0.5, 300 + seed)
    s[D // 3] = 0.0
    return s


GEGLU_SHAPES = [(1, 8), (300, 512), (1537, 264), (4100, 264), (1537, 2056), (2561, 4096)]


def geglu_inputs(M: int, F: int, seed: int = 0):
    """h (M, 2F): values N(0, 2); gates: even rows a sweep over [-14, 14] with +0 and -0 planted, odd rows N(0, 1.5).
    d (M, F): N(0, 2). bf16 values in float64; the sign of -0 is lost in float64, so the gate tensor is also returned
    as bf16 (``h_bf16``) for the kernel."""
    a = randn_bf16((M, F), 2.0, 400 + seed)
    g = torch.randn((M, F), generator=torch.Generator().manual_seed(401 + seed), dtype=torch.float64) * 1.5
    sweep = torch.linspace(-14.0, 14.0, F, dtype=torch.float64).roll(3)
    ev = torch.arange(M) % 2 == 0
    g[ev] = sweep * (1.0 - 0.05 * (torch.arange(int(ev.sum()), dtype=torch.float64).view(-1, 1) % 8))
    h16 = torch.cat([a, g], dim=-1).to(torch.bfloat16)
    h16[0, F] = 0.0
    h16[0, F + min(1, F - 1)] = -0.0
    d = randn_bf16((M, F), 2.0, 402 + seed)
    return h16, h16.double(), d


XENT_GSCALES = (1.0, 0.25, 1.0 / (1.5 * 12288))
XENT_PAD_V, XENT_PAD_FROM, XENT_PAD_LOGIT = 32512, 32356, -3.0e4


def xent_form(V: int) -> int:
    """which kernel ``xent_colsum_`` selects (csrc/kernels/xent.hip): 2 / 1 register-resident, 0 LDS accumulator."""
    if V % 8 == 0 and V <= 8192:
        return 2
    if V % 4 == 0 and V <= 32768:
        return 1
    return 0


def xent_label_kinds(V: int, row: int):
    """the columns a label is planted at for ``row``: 0, V - 1, and by form the edges of the row's unaligned head,
    vector body and scalar tail (form 0) or of a lane's vector and a wave's span (register forms)."""
    form = xent_form(V)
    lim = XENT_PAD_FROM if V == XENT_PAD_V else V
    cols = [0, lim - 1]
    if form == 0:
        head = min((8 - ((row * V) & 7)) & 7, V)
        nvec = (V - head) // 8
        cols += [head - 1, head, head + 8 * nvec - 1] + list(range(head + 8 * nvec, V))
    else:
        E, W = (8, 4) if form == 2 else (4, 16)
        cols += [E, 2 * E - 1, 64 * E - 1, 64 * E, W * 64 * E - 1, W * 64 * E]
    return list(dict.fromkeys(c for c in cols if 0 <= c < lim))


def xent_inputs(R: int, V: int, rot: int = 0, seed: int = 0):
    """-> (logits (R, V) bf16 values, labels (R,)). Row r's label is ``xent_label_kinds(V, r)[(r + rot) % len]``; its
    kind is (r + rot) % 6: N(0, 3); the label logit leads by 20; a non-label logit leads by 20; all equal (loss = ln V);
    offset +80; offset -80. At V = 32512 the columns from 32356 on are -3e4 (the assembly head's padding)."""
    g = torch.Generator().manual_seed(500 + seed + 7 * rot)
    x = torch.randn(R, V, generator=g, dtype=torch.float64) * 3.0
    labels = torch.empty(R, dtype=torch.long)
    lim = XENT_PAD_FROM if V == XENT_PAD_V else V
    for r in range(R):
        kinds = xent_label_kinds(V, r)
        lab = kinds[(r + rot) % len(kinds)]
        labels[r] = lab
        kind = (r + rot) % 6
        if kind == 1:
            x[r, lab] = x[r, :lim].max() + 20.0
        elif kind == 2:
            other = (lab + 1 + lim // 2) % lim
            x[r, other if other != lab else (lab + 1) % lim] = x[r, :lim].max() + 20.0
        elif kind == 3:
            x[r] = 1.25
        elif kind == 4:
            x[r] += 80.0
        elif kind == 5:
            x[r] -= 80.0
    if V == XENT_PAD_V:
        x[:, XENT_PAD_FROM:] = XENT_PAD_LOGIT
    return bf16_round(x), labels


def embed_run_ids(V: int, runs=(1, 63, 64, 65, 128, 129, 500), seed: int = 0):
    """ids with runs of exactly the given lengths of equal ids (the chunk boundaries of ``embed_bwd_``), shuffled."""
    g = torch.Generator().manual_seed(600 + seed)
    table_rows = torch.randperm(V, generator=g)[:len(runs)]
    ids = torch.cat([torch.full((L,), int(t), dtype=torch.long) for L, t in zip(runs, table_rows)])
    return ids[torch.randperm(ids.numel(), generator=g)]
