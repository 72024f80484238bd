"""K20: every VQGAN decoder kernel of ``csrc/kernels/conv.hip`` on its own, element by element, against the float64
references of ``tests/vqgan_ref.py`` (pinned to torch by ``test_vqgan_ref_cpu.py``).

The references read exactly what the kernel reads (bf16 activations / weights, fp32 statistics, upcast), so every
bound below is the kernel's own arithmetic: u = 2^-24 (fp32 rounding), 2^-8 (one rounding to bf16), and the
magnitude convolution A = conv(|x'|, |w|) + |bias| + |res| for worst-case accumulation. GroupNorm inputs are the
float64 reference statistics cast to fp32, never ``gn_stats``' output, so each kernel is judged alone. Image n of a
batch is (n + 1) * randn + 2 n: a table indexed with the wrong image is far outside every bound.

Constants that are measured rather than derived (never from a kernel's output):

| constant        | value      | measured between                                                    | factor |
|-----------------|------------|---------------------------------------------------------------------|--------|
| C_GN_MEASURED   | 3.535e-05  | ``vqgan_ref.measure_gn_constant()``: max |R32 - R| / A over the     |        |
|                 |            | GroupNorm conv cases, R32 / R = the round_act emulation with        |        |
|                 |            | SiLU(GN(x)) evaluated in fp32 / float64 on the CPU                  |        |
| C_GN            | 1.414e-04  | = 4 x C_GN_MEASURED: the flips of the activation's bf16 rounding    | 4      |

The 2^-20 * A term of ``conv_out`` (fast rcp / exp2 in SiLU) is derived, see ``test_conv_out``.
"""
import math

import pytest
import torch

import vqgan_ref as vr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = 2.0 ** -8
C_GN_MEASURED = 3.535e-05
C_GN = 4 * C_GN_MEASURED
EPS = 1e-6


@pytest.fixture(scope="module")
def ext(cuda):
    from dalle_amd.ops.ext import load_extension

    return load_extension(required=True)


def conv_bound(r, a, k, gn):
    """|y - R| <= 2^-8 |R| (one bf16 output rounding) + (K + 2) u A (fp32 accumulation of K products, bias,
    residual) [+ C_GN A with GroupNorm: R is the round_act reference]."""
    return BF * r.abs() + ((k + 2) * U + (C_GN if gn else 0.0)) * a


def _index(flat, shape):
    idx = []
    for s in reversed(shape):
        idx.append(flat % s)
        flat //= s
    return tuple(reversed(idx))


def assert_within(got, ref, bound, what, border_hw=None):
    """Per element |got - ref| <= bound; reports the worst element (and, for images, whether it is a border pixel)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    flat = int(ratio.argmax())
    idx = _index(flat, tuple(ref.shape))
    where = ""
    if border_hw is not None:
        (ay, ax), (h, w) = border_hw
        on = idx[ay] in (0, h - 1) or idx[ax] in (0, w - 1)
        where = ", on the image border" if on else ", interior"
    bad = int((err > bound).sum())
    msg = (f"{what}: worst element {idx}{where}: got {got.flatten()[flat].item():.9g} ref {ref.flatten()[flat].item():.9g} "
           f"err {err.flatten()[flat].item():.3g} bound {bound.flatten()[flat].item():.3g} "
           f"(err / bound {ratio.flatten()[flat].item():.3f}); {bad} of {err.numel()} elements out of bound")
    print(msg)
    assert bad == 0, msg


def _dev(t, dev):
    return None if t is None else t.to(dev).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# conv3x3
@pytest.mark.parametrize("case", vr.conv_cases(), ids=lambda c: "-".join(str(int(v)) for v in c))
def test_conv3x3(cuda, ext, case):
    n, h, w, cin, cout, ups, gn, _, _ = case
    d = vr.make_conv_case(case, EPS)
    ref, a = vr.conv3x3_ref(d["x"], d["w"], d["bias"], d["res"], gn=d["gn"], ups=ups, round_act=True)
    args = [_dev(d["x"], cuda), _dev(d["w"], cuda), _dev(d["bias"], cuda), _dev(d["res"], cuda)]
    if gn:
        args += [_dev(t, cuda) for t in d["gn"]]
    y = ext.conv3x3(*args, ups=ups)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (n, h, w, cout)
    assert_within(y, ref, conv_bound(ref, a, 9 * cin, gn), f"conv3x3 {case}", border_hw=((1, 2), (h, w)))


@pytest.mark.parametrize("n,h,w,cin,cout", [(1, 8, 16, 96, 128), (1, 8, 16, 64, 64), (1, 8, 24, 64, 128),
                                             (1, 8, 16, 1088, 128)])
def test_conv3x3_rejects(cuda, ext, n, h, w, cin, cout):
    x = torch.zeros(n, h, w, cin, device=cuda, dtype=torch.bfloat16)
    wk = torch.zeros(cout, 9 * cin, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.conv3x3(x, wk)


# ---------------------------------------------------------------------------------------------------------------
# gn_stats
GN_C = [32, 96, 128, 192, 512, 2048]
GN_HW = [(1, 1), (1, 7), (7, 9), (8, 8), (5, 13), (16, 16), (25, 40)]
GN_STATS_CASES = sorted({(c, hw) for c in GN_C for hw in [(7, 9), (16, 16)]} | {(96, hw) for hw in GN_HW})


def _gn_stats_bounds(x, c, hw):
    """n_t = additions per fp32 accumulator: a workgroup takes ceil(HW / 64) pixels, 256 / (C / 8) of them per pass.
    |dmean| <= (n_t + 4) u E|x|; |dvar| <= (n_t + 6) u (E[x^2] + 2 |mu| E|x|) (var = Q / cnt - mu^2);
    |drstd| / rstd <= 0.5 dvar / (var + eps), plus 1.5 u for what no implementation can avoid: the fp32 rounding of
    the returned rstd (u) and of eps itself (u / 2)."""
    mean, rstd, eabs, esq = vr.gn_stats_ref(x, EPS)
    n_t = math.ceil(math.ceil(hw / 64) / (256 // (c // 8)))
    var = (rstd ** -2 - EPS).clamp_min(0.0)
    dmean = (n_t + 4) * U * eabs
    dvar = (n_t + 6) * U * (esq + 2 * mean.abs() * eabs)
    drstd = (0.5 * dvar / (var + EPS) + 1.5 * U) * rstd
    return mean, rstd, dmean, drstd


@pytest.mark.parametrize("c,hw", GN_STATS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gn_stats(cuda, ext, c, hw):
    """mean AND rstd of groups whose mean / std ratio is 0, 4 and 16 (the variance is Q / cnt - mu^2 from fp32
    partial sums), with empty pixel chunks (HW < 64), C / 8 not dividing 256, and one pixel per pass (C = 2048)."""
    n, (h, w) = 3, hw
    g = torch.Generator().manual_seed(c * 1000 + h * w)
    ratio = torch.tensor([0.0, 4.0, 16.0])[torch.arange(32) % 3].repeat_interleave(c // 32)
    scale = torch.arange(1, n + 1, dtype=torch.float32)[:, None, None, None]
    x = ((torch.randn(n, h, w, c, generator=g) + ratio) * scale).to(torch.bfloat16)
    mean, rstd, dmean, drstd = _gn_stats_bounds(x, c, h * w)
    m, r = ext.gn_stats(x.to(cuda), EPS)
    assert m.dtype == r.dtype == torch.float32 and tuple(m.shape) == tuple(r.shape) == (n, 32)
    assert_within(m, mean, dmean, f"gn_stats mean C={c} HW={h}x{w}")
    assert_within(r, rstd, drstd, f"gn_stats rstd C={c} HW={h}x{w}")


@pytest.mark.parametrize("c,hw", [(96, (7, 9)), (2048, (16, 16)), (32, (1, 1))], ids=lambda v: str(v).replace(" ", ""))
def test_gn_stats_constant_input(cuda, ext, c, hw):
    x = torch.full((3, hw[0], hw[1], c), 3.0, dtype=torch.bfloat16)
    mean, rstd, dmean, drstd = _gn_stats_bounds(x, c, hw[0] * hw[1])
    assert (rstd - EPS ** -0.5).abs().max().item() < 1e-6
    m, r = ext.gn_stats(x.to(cuda), EPS)
    assert_within(m, mean, dmean, f"gn_stats mean of a constant C={c}")
    assert_within(r, rstd, drstd, f"gn_stats rstd of a constant C={c}")


@pytest.mark.parametrize("c", [48, 2080])
def test_gn_stats_rejects(cuda, ext, c):
    with pytest.raises(RuntimeError, match="unsupported channel count"):
        ext.gn_stats(torch.zeros(1, 2, 2, c, device=cuda, dtype=torch.bfloat16), EPS)


# ---------------------------------------------------------------------------------------------------------------
# gn_apply
def _gn_inputs(n, h, w, c, seed, gamma_value=None):
    g = torch.Generator().manual_seed(seed)
    nn = torch.arange(n, dtype=torch.float32)[:, None, None, None]
    x = ((nn + 1) * torch.randn(n, h, w, c, generator=g) + 2 * nn).to(torch.bfloat16)
    gamma = torch.rand(c, generator=g) + 0.5 if gamma_value is None else torch.full((c,), float(gamma_value))
    beta = torch.rand(c, generator=g) * 0.6 - 0.3
    mean, rstd, _, _ = vr.gn_stats_ref(x, EPS)
    return x, mean.float(), rstd.float(), gamma, beta


def _gn_apply_bound(x, mean, rstd, gamma, beta, ref):
    """2^-8 |ref| (the bf16 output) + 8 u (|x - mean| rstd |gamma| + |beta|): four fp32 roundings of the affine
    form, doubled. Through SiLU the same absolute term holds (|silu'| <= 1.1)."""
    c = x.shape[-1]
    pre = (x.double() - vr._per_channel(mean, c, torch.float64)).abs() * vr._per_channel(rstd, c, torch.float64)
    return BF * ref.abs() + 8 * U * (pre * gamma.double().abs() + beta.double().abs())


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("n,h,w,c", [(1, 1, 3, 32), (3, 5, 7, 96), (2, 16, 16, 512)])
def test_gn_apply(cuda, ext, n, h, w, c, silu):
    """Vector counts off a multiple of 256, and (C = 96) one 8-channel vector spanning three groups."""
    x, mean, rstd, gamma, beta = _gn_inputs(n, h, w, c, seed=c + h)
    ref = vr.gn_apply_ref(x, mean, rstd, gamma, beta, silu)
    y = ext.gn_apply(x.to(cuda), mean.to(cuda), rstd.to(cuda), gamma.to(cuda), beta.to(cuda), silu=silu)
    assert y.dtype == torch.bfloat16
    assert_within(y, ref, _gn_apply_bound(x, mean, rstd, gamma, beta, ref), f"gn_apply {(n, h, w, c)} silu={silu}")


@pytest.mark.parametrize("silu", [False, True])
def test_gn_apply_large_activations(cuda, ext, silu):
    """gamma = 50: activations reach +-100 and beyond; exp2 of the large negatives overflows inside SiLU and the
    result must still be a finite value within the bound of 0."""
    x, mean, rstd, gamma, beta = _gn_inputs(3, 5, 7, 96, seed=11, gamma_value=50.0)
    pre = vr.gn_apply_ref(x, mean, rstd, gamma, beta, False)
    assert pre.max().item() > 100 and pre.min().item() < -100
    ref = vr.gn_apply_ref(x, mean, rstd, gamma, beta, silu)
    bound = _gn_apply_bound(x, mean, rstd, gamma, beta, ref)
    y = ext.gn_apply(x.to(cuda), mean.to(cuda), rstd.to(cuda), gamma.to(cuda), beta.to(cuda), silu=silu)
    assert_within(y, ref, bound, f"gn_apply gamma=50 silu={silu}")
    if silu:
        neg = pre < -90
        assert neg.any() and (y.double().cpu()[neg].abs() <= bound[neg]).all()


# ---------------------------------------------------------------------------------------------------------------
# softmax_rows
def _softmax_rows(kind, r, l, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(r, l, generator=g)
    if kind == "big":
        s = s * 1e4
    elif kind == "constant":
        s = torch.arange(r, dtype=torch.float32)[:, None].expand(r, l) + 0.5
    elif kind == "onehot":
        s[torch.arange(r), (torch.arange(r) * 7) % l] += 20.0
    return s.contiguous()


def _check_softmax(ext, cuda, s, scale, what):
    """|p - ref| <= (2^-8 + 2^-22 max|s scale|) ref + 2^-126: the bf16 output, four fp32 roundings of an exponent of
    that size, and flush-to-zero below the smallest normal; every row sums to 1 within 2^-8."""
    ref = vr.softmax_rows_ref(s, scale)
    sc32 = torch.tensor(float(scale), dtype=torch.float32).double()
    big = (s.double() * sc32).abs().amax(dim=-1, keepdim=True)
    p = ext.softmax_rows(s.to(cuda), scale)
    assert p.dtype == torch.bfloat16 and p.shape == s.shape
    assert_within(p, ref, (BF + 4 * U * big) * ref + 2.0 ** -126, what)
    rowsum = p.double().cpu().sum(-1)
    assert (rowsum - 1).abs().max().item() <= BF, (what, rowsum)


@pytest.mark.parametrize("kind", ["gaussian", "big", "constant", "onehot"])
@pytest.mark.parametrize("scale", [1.0, 512 ** -0.5, 0.0])
@pytest.mark.parametrize("l", [1, 63, 64, 255, 256, 257, 1000, 1024])
def test_softmax_rows(cuda, ext, l, scale, kind):
    for r in (1, 5):
        _check_softmax(ext, cuda, _softmax_rows(kind, r, l, seed=l + r), scale, f"softmax_rows {kind} R={r} L={l} scale={scale}")


def test_softmax_rows_keeps_3d_shape(cuda, ext):
    s = _softmax_rows("onehot", 128, 64, seed=5).view(2, 64, 64)
    _check_softmax(ext, cuda, s, 512 ** -0.5, "softmax_rows (2, 64, 64)")


# ---------------------------------------------------------------------------------------------------------------
# conv_out
def _conv_out_inputs(n, h, w, c, bias):
    x, mean, rstd, gamma, beta = _gn_inputs(n, h, w, c, seed=h * w + c)
    g = torch.Generator().manual_seed(c)
    wk = ((torch.rand(3, 9 * c, generator=g) * 2 - 1) / math.sqrt(9 * c)).to(torch.bfloat16)
    b = (torch.rand(3, generator=g) - 0.5) if bias is None else torch.tensor(bias, dtype=torch.float32)
    return x, wk, b, mean, rstd, gamma, beta


@pytest.mark.parametrize("bias", [None, (3.0, -3.0, 0.0)], ids=["bias", "saturating"])
@pytest.mark.parametrize("n,h,w,c", [(2, 5, 7, 32), (1, 16, 16, 96), (2, 17, 33, 128), (1, 40, 24, 64)])
def test_conv_out(cuda, ext, n, h, w, c, bias):
    """The kernel is fp32 end to end. On the pre-clamp value v (recovered exactly as 2 img - 1):
    |v - ref| <= (27 C + 4) u A + 2^-20 A, compared after the (1-Lipschitz) clamp so it covers every element.

    The 2^-20 A term is for SiLU's fast rcp / exp2, both accurate to 1 ulp (2 u relative): silu(t) =
    t * rcp(1 + exp2(-t log2 e)) carries 2 u (exp2) + 2 u (rcp) + u (the sum) + u (the product) plus the exponent's
    two roundings, 2 u |t| * e^-t / (1 + e^-t), i.e. (6 + 2 |t| s(-t)) u relative. |t| s(-t) exceeds 5 only where
    |silu(t)| < 0.034, so weighted by the activations' magnitudes it stays below 16 u = 2^-20 of A; the strict
    remainder is inside the first term, which allows 27 C + 4 roundings where the two 4.5 C-long FMA chains, the
    bias and their sum make 4.5 C + 2.

    With bias (+3, -3, 0) both clamp sides saturate: exactly 1.0 / 0.0 wherever the reference is beyond +-1 by more
    than the bound. Sides below one 16-pixel tile, off tile multiples, and 1 to 4 channel chunks."""
    x, wk, b, mean, rstd, gamma, beta = _conv_out_inputs(n, h, w, c, bias)
    pre, _, a = vr.conv_out_ref(x, wk, b, mean, rstd, gamma, beta)
    bound = ((27 * c + 4) * U + 2.0 ** -20) * a
    img = ext.conv_out(*[t.to(cuda) for t in (x, wk, b, mean, rstd, gamma, beta)])
    assert img.dtype == torch.float32 and tuple(img.shape) == (n, 3, h, w)
    got = img.double().cpu()
    assert_within(2 * got - 1, pre.clamp(-1, 1), bound, f"conv_out {(n, h, w, c)} bias={bias}", border_hw=((2, 3), (h, w)))
    hi, lo = pre > 1 + bound, pre < -1 - bound
    if bias is not None:
        assert hi.any() and lo.any() and (pre.abs() < 1).any()
    assert (got[hi] == 1.0).all() and (got[lo] == 0.0).all()


@pytest.mark.parametrize("c", [160, 48])
def test_conv_out_rejects(cuda, ext, c):
    z = lambda *s: torch.zeros(*s, device=cuda)  # noqa: E731
    with pytest.raises(RuntimeError, match="conv_out"):
        ext.conv_out(z(1, 4, 4, c).bfloat16(), z(3, 9 * c).bfloat16(), z(3), z(1, 32), z(1, 32), z(c), z(c))
