"""K19: the VQGAN encoder kernels of ``csrc/kernels/conv.hip`` that the decoder does not have --
``conv3x3(down=True)``, ``conv_in_rgb``, ``linear_argmax`` -- each on its own against the float64 references of
``tests/vqgan_enc_ref.py`` (pinned to torch by ``test_vqgan_enc_ref_cpu.py``).

As in ``test_vqgan_kernels_gpu.py`` the references read exactly what the kernel reads, so every bound is the kernel's
own arithmetic: u = 2^-24 (fp32 rounding), 2^-8 (one rounding to bf16) and the magnitude sums A for worst-case fp32
accumulation in any order. Nothing here is measured from a kernel's output.
"""
import pytest
import torch

import vqgan_enc_ref as er
from test_vqgan_kernels_gpu import BF, U, assert_within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext(cuda):
    from dalle_amd.ops.ext import load_extension

    return load_extension(required=True)


def _dev(t, dev):
    return None if t is None else t.to(dev).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# conv3x3(down=True)
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", er.DOWN_SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_conv3x3_down(cuda, ext, shape, has_bias):
    """|y - R| <= 2^-8 |R| + (9 Cin + 2) u A. (1, 2, 256): every output pixel reads the bottom pad row;
    (1, 256, 2): every output pixel reads the right pad column; image n is (n + 1) randn + 2 n."""
    n, h, w, cin, cout = shape
    x, wk, bias = er.make_down_case(shape, has_bias)
    ref, a = er.conv_down_ref(x, wk, bias)
    y = ext.conv3x3(_dev(x, cuda), _dev(wk, cuda), _dev(bias, cuda), down=True)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (n, h // 2, w // 2, cout)
    assert_within(y, ref, BF * ref.abs() + (9 * cin + 2) * U * a, f"conv3x3 down {shape} bias={has_bias}",
                  border_hw=((1, 2), (h // 2, w // 2)))


def test_conv3x3_down_rejects(cuda, ext):
    def z(*s):
        return torch.zeros(*s, device=cuda, dtype=torch.bfloat16)

    wk = z(128, 9 * 128)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.conv3x3(z(1, 17, 32, 128), wk, down=True)  # odd H
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.conv3x3(z(1, 32, 17, 128), wk, down=True)  # odd W
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.conv3x3(z(1, 16, 16, 128), wk, down=True)  # 64 output pixels
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.conv3x3(z(1, 16, 32, 128), wk, ups=True, down=True)
    f = lambda *s: torch.ones(*s, device=cuda)  # noqa: E731
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.conv3x3(z(1, 16, 32, 128), wk, None, None, f(1, 32), f(1, 32), f(128), f(128), down=True)  # GroupNorm
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.conv3x3(z(1, 16, 32, 128), wk, None, z(1, 8, 16, 128), down=True)  # residual


# ---------------------------------------------------------------------------------------------------------------
# conv_in_rgb
@pytest.mark.parametrize("shape", er.RGB_SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_conv_in_rgb(cuda, ext, shape):
    """|y - R| <= 2^-8 |R| + 29 u A against R from x' = bf16(fp32(2 x - 1)): 27 products and the bias in fp32, one
    rounding to bf16. The pictures contain exact 0.0 and 1.0; one-pixel-high and one-pixel-wide pictures have every
    pixel on two borders."""
    n, h, w, cout = shape
    img, wk, bias = er.make_rgb_case(shape)
    assert (img == 0).any() and (img == 1).any() and img.min() >= 0 and img.max() <= 1
    ref, a = er.conv_in_rgb_ref(img, wk, bias)
    y = ext.conv_in_rgb(_dev(img, cuda), _dev(wk, cuda), _dev(bias, cuda))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (n, h, w, cout)
    assert_within(y, ref, BF * ref.abs() + 29 * U * a, f"conv_in_rgb {shape}", border_hw=((1, 2), (h, w)))


@pytest.mark.parametrize("h,w,cout", [(8, 16, 64), (8, 8, 128), (8, 16, 192)])
def test_conv_in_rgb_rejects(cuda, ext, h, w, cout):
    img = torch.zeros(1, 3, h, w, device=cuda)
    wk = torch.zeros(cout, 27, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.conv_in_rgb(img, wk, torch.zeros(cout, device=cuda))


# ---------------------------------------------------------------------------------------------------------------
# linear_argmax
@pytest.fixture(scope="module")
def argmax_refs():
    """The float64 logits, magnitudes and inputs of every shape, computed once and left unchanged."""
    out = {}
    for shape in er.ARGMAX_SHAPES:
        x, w, bias = er.make_argmax_case(shape)
        r, a = er.linear_argmax_ref(x, w, bias)
        out[shape] = (x, w, bias, r, a)
    return out


def _winner_columns(m, v):
    """One planted column per row, in turn from: the first column tile (its first and last column), the middle tile,
    the last tile (its second and its last column). The last row -- in the masked tail tile of rows when M is no
    multiple of 128 -- gets the very last column."""
    mid, last = (v // 128) // 2, v // 128 - 1
    pool = sorted({0, 127, mid * 128 + 64, last * 128 + 1, v - 1})
    cols = torch.tensor([pool[i % len(pool)] for i in range(m)])
    cols[-1] = v - 1
    return cols, pool


@pytest.mark.parametrize("shape", er.ARGMAX_SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_linear_argmax_near_optimal(cuda, ext, argmax_refs, shape):
    """With b_j = (K + 2) u A_j (fp32 accumulation of K products and the bias, any order), the float64 logit of the
    returned column is within b[got] + b[argmax r] of the row's maximum -- every row, no exemptions."""
    m, k, v = shape
    x, w, bias, r, a = argmax_refs[shape]
    got = ext.linear_argmax(_dev(x, cuda), _dev(w, cuda), _dev(bias, cuda))
    assert got.dtype == torch.int64 and tuple(got.shape) == (m,)
    got = got.cpu()
    assert got.min() >= 0 and got.max() < v
    b = (k + 2) * U * a
    best = r.argmax(1)
    rows = torch.arange(m)
    gap = r[rows, best] - r[rows, got]
    allow = b[rows, got] + b[rows, best]
    worst = int((gap / allow).argmax())
    agree = (got == best).float().mean().item()
    msg = (f"linear_argmax {shape}: {agree:.4f} of rows equal the float64 argmax; worst row {worst}: got column "
           f"{int(got[worst])} (r {r[worst, got[worst]].item():.9g}) best {int(best[worst])} (r {r[worst, best[worst]].item():.9g}) "
           f"gap {gap[worst].item():.3g} allowed {allow[worst].item():.3g}; {int((gap > allow).sum())} of {m} rows out of bound")
    print(msg)
    assert (gap <= allow).all(), msg


@pytest.mark.parametrize("shape", er.ARGMAX_SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_linear_argmax_planted_winners(cuda, ext, argmax_refs, shape):
    """Every row gets one column lifted above its runner-up by at least 100 max b and must return exactly that
    column. The kernel's bias is per column, so the per-row lift goes through the operands: the last features of x
    and w are zeroed, planted column c gets ``w[c, K - 1 - class(c)] = lift`` and a row switches on the feature of
    its own column's class, ``x[i, K - 1 - class] = 1`` -- 1 * lift is exact in bf16 and fp32, so this adds the
    lift to that one logit of the row and nothing anywhere else."""
    m, k, v = shape
    x, w, bias, _, _ = argmax_refs[shape]
    cols, pool = _winner_columns(m, v)
    xs, ws = x.clone(), w.clone()
    xs[:, k - len(pool):] = 0
    ws[:, k - len(pool):] = 0
    r0, a0 = er.linear_argmax_ref(xs, ws, bias)
    lift = (r0.max() - r0.min()).item() + 200 * ((k + 2) * U * a0).max().item() + 1.0
    lift = torch.tensor(1.02 * lift).to(torch.bfloat16)  # a bf16 operand; 2 % covers its rounding (checked below)
    for t, c in enumerate(pool):
        ws[c, k - 1 - t] = lift
        xs[cols == c, k - 1 - t] = 1.0
    r, a = er.linear_argmax_ref(xs, ws, bias)
    top2 = r.topk(2, dim=1)
    need = 100 * ((k + 2) * U * a).max().item()
    assert torch.equal(top2.indices[:, 0], cols) and (top2.values[:, 0] - top2.values[:, 1]).min().item() >= need, \
        "test construction: the planted column must lead every row by 100 max b"
    got = ext.linear_argmax(_dev(xs, cuda), _dev(ws, cuda), _dev(bias, cuda)).cpu()
    wrong = (got != cols).nonzero().flatten().tolist()
    print(f"linear_argmax planted {shape}: columns {pool}, lift {lift.item()}, margin needed {need:.3g}, "
          f"{len(wrong)} of {m} rows wrong")
    assert not wrong, (wrong[:10], got[wrong[:10]].tolist(), cols[wrong[:10]].tolist())
    assert int(got[-1]) == v - 1


TIE_CASES = [(s, "same_tile") for s in er.ARGMAX_SHAPES] + [(s, "other_tile") for s in er.ARGMAX_SHAPES if s[2] >= 256]


@pytest.mark.parametrize("shape,where", TIE_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(str(d) for d in v))
def test_linear_argmax_ties_go_to_the_lowest_index(cuda, ext, argmax_refs, shape, where):
    """Two identical weight rows with identical biases, lifted above everything else: the two logits are the same
    fp32 operations on the same values, bitwise equal, so the lower index must come back for every row -- once with
    both columns inside the last column tile, once with them in the first and the last tile."""
    m, k, v = shape
    x, w, bias, r, a = argmax_refs[shape]
    lo, hi = (v - 128 + 5, v - 128 + 77) if where == "same_tile" else (37, v - 3)
    wb, bb = w.clone(), bias.clone()
    wb[hi] = wb[lo]
    lift = 2.0 * (r.max() - r.min()).item() + 100 * ((k + 2) * U * a).max().item() + 1.0
    bb[lo] = bb[hi] = lift
    got = ext.linear_argmax(_dev(x, cuda), _dev(wb, cuda), _dev(bb, cuda)).cpu()
    assert (got == lo).all(), (where, lo, hi, got.unique().tolist())


@pytest.mark.parametrize("m,k,v", [(4, 32, 128), (4, 96, 128), (4, 64, 64), (4, 64, 192)])
def test_linear_argmax_rejects(cuda, ext, m, k, v):
    z = torch.zeros
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.linear_argmax(z(m, k, device=cuda, dtype=torch.bfloat16), z(v, k, device=cuda, dtype=torch.bfloat16),
                          z(v, device=cuda))
