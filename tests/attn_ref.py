"""Float64 reference of the sparse attention family (K7a-e, D7) on the kernels' padded storage layout, and the seeded
inputs of ``test_attention_kernels_gpu.py``. No GPU code: plain torch in float64, pinned to ``ops.reference`` +
autograd and to a brute-force mask by ``test_attn_ref_cpu.py``. It may run on any torch device.

Layout (``models/patterns.py``): q / k / v are ``(B*H, Np, 64)``; storage rows ``[0, T)`` are the text positions,
``[T, Tp)`` padding, ``[Tp, Np)`` the ``S*S`` image tokens (column-major for ``axial_col``), the row of the dropped
last image token included. ``out`` and its gradient are token-major ``(B, n, H*64)``.

The reference reads what the kernels read: q (pre-scaled by 1/8), k, v, dO as bf16 values upcast, and for the
backward the forward's bf16 ``out`` (``delta = rowsum(dO * bf16(out))``). ``lse`` is in the kernels' convention:
``log2(sum_j exp(s_ij))`` per storage row.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from dalle_amd.models.patterns import AttnGeometry, allowed, storage_index
from dalle_amd.models.rotary import apply_rotary, apply_rotary_inverse, rotary_tables, rotate_pairs

LOG2E = 1.0 / math.log(2.0)
QSCALE = 0.125
POISON = 4.0           # padding rows of K and V (the kernels mask them; they must not need zeros)
RESCALE_THR = 8.0      # attention.hip: the forward's lazy rescale threshold, log2 units


@dataclass(frozen=True)
class Case:
    T: int
    S: int
    attn_type: str
    K: int = 5
    B: int = 1
    H: int = 3

    @property
    def geom(self) -> AttnGeometry:
        return AttnGeometry(self.T, self.S, self.K)

    @property
    def n(self) -> int:
        return self.geom.seq_len

    @property
    def Tp(self) -> int:
        return self.geom.text_pad

    @property
    def Np(self) -> int:
        return self.geom.padded_len

    @property
    def BH(self) -> int:
        return self.B * self.H

    def __str__(self):
        k = f"-K{self.K}" if self.attn_type == "conv_like" else ""
        return f"T{self.T}-S{self.S}-{self.attn_type}{k}-B{self.B}H{self.H}"


# ---------------------------------------------------------------------------------------------------------------
# layout
def seq_to_storage(case: Case) -> torch.Tensor:
    """(n,) storage row of every real sequence position."""
    return storage_index(case.geom, case.attn_type)[:case.n]


def storage_to_seq(case: Case) -> torch.Tensor:
    """(Np,) sequence position of every storage row, -1 for padding rows and the dropped last image token."""
    s2q = torch.full((case.Np,), -1, dtype=torch.long)
    s2q[seq_to_storage(case)] = torch.arange(case.n)
    return s2q


def pack(x: torch.Tensor, case: Case, fill: float = 0.0) -> torch.Tensor:
    """(B, H, n, 64) -> (B*H, Np, 64); rows that hold no sequence position get ``fill``."""
    B, H, n, D = x.shape
    out = torch.full((B * H, case.Np, D), fill, dtype=x.dtype, device=x.device)
    out[:, seq_to_storage(case).to(x.device)] = x.reshape(B * H, n, D)
    return out


def unpack(xs: torch.Tensor, case: Case) -> torch.Tensor:
    """(B*H, Np, ...) -> (B, H, n, ...)."""
    y = xs[:, seq_to_storage(case).to(xs.device)]
    return y.reshape(case.B, case.H, case.n, *xs.shape[2:])


def tokens_to_heads(x: torch.Tensor, H: int) -> torch.Tensor:
    """token-major (B, n, H*64) -> (B, H, n, 64)."""
    B, n, HD = x.shape
    return x.reshape(B, n, H, HD // H).transpose(1, 2)


def heads_to_tokens(x: torch.Tensor) -> torch.Tensor:
    """(B, H, n, 64) -> token-major (B, n, H*64)."""
    B, H, n, D = x.shape
    return x.transpose(1, 2).reshape(B, n, H * D)


def storage_mask(case: Case) -> torch.Tensor:
    """(Np, Np) bool: storage query row i may attend storage key row j. Rows / columns without a sequence
    position are all False."""
    s2q = storage_to_seq(case)
    real = s2q >= 0
    p = s2q.clamp(min=0)
    m = allowed(case.geom, case.attn_type, p.view(-1, 1), p.view(1, -1))
    return m & real.view(-1, 1) & real.view(1, -1)


def describe_row(case: Case, s: int) -> str:
    """storage row -> sequence position -> image row / col, for failure messages."""
    p = int(storage_to_seq(case)[s])
    if s < case.Tp:
        return f"storage row {s} -> " + (f"text position {p}" if p >= 0 else "text padding")
    kk = (p if p >= 0 else case.n) - case.T
    tail = "" if p >= 0 else " (dropped last image token)"
    return (f"storage row {s} (tile {s // 32} lane {s % 32}) -> position {p if p >= 0 else case.n} -> "
            f"image row {kk // case.S} col {kk % case.S}{tail}")


# ---------------------------------------------------------------------------------------------------------------
# the reference
def attention_ref(q, k, v, case: Case, dO=None, out_bf16=None, extra=None, mags=True):
    """q, k, v (and dO): float64 ``(B*H, Np, 64)`` storage layout. Returns a dict:

    ``O``, ``lse`` (log2 domain), ``P`` (normalised, zero on padding rows), ``real`` (Np,) bool and the magnitude
    terms ``A_o = sum_j P_ij |v_jd|``, ``smax_i = max_j sum_d |q_id||k_jd|`` over the allowed keys; with ``dO``
    (zero on padding rows) also ``dQ``, ``dK``, ``dV``, ``dS``, ``delta`` and ``A_dv = sum_i P_ij |dO_id|``,
    ``A_dq = sum_j |dS_ij||k_jd|``, ``A_dk = sum_i |dS_ij||q_id|``, ``OdO_i = sum_d |O_id||dO_id|``,
    ``dOv_ij = sum_d |dO_id||v_jd|``, ``D_ij = |dP_ij - delta_i|`` on the allowed pairs. ``out_bf16``: the bf16 forward output (storage layout, upcast) that the kernels
    form ``delta`` from; None: the exact ``O`` (the autograd gradient). ``extra``: (Np, Np) bool of additionally
    admitted pairs (the sensitivity test)."""
    dev = q.device
    mask = storage_mask(case)
    if extra is not None:
        mask = mask | extra
    mask = mask.to(dev)
    real = (storage_to_seq(case) >= 0).to(dev)
    s = q @ k.transpose(-1, -2)
    s = s.masked_fill(~mask, -math.inf)
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    P = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
    lse = ((m + torch.log(l.clamp_min(1e-300))) * LOG2E).squeeze(-1)
    lse = torch.where(real, lse, torch.zeros_like(lse))
    r = {"O": P @ v, "lse": lse, "P": P, "real": real, "scores": s}
    if mags:
        r["A_o"] = P @ v.abs()
        r["vabs_sum"] = v.abs().sum(dim=1, keepdim=True)
        sa = (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(~mask, 0.0)
        r["smax"] = sa.max(dim=-1).values
    if dO is None:
        return r
    Ob = r["O"] if out_bf16 is None else out_bf16
    delta = (dO * Ob).sum(-1, keepdim=True)
    dP = dO @ v.transpose(-1, -2)
    dS = P * (dP - delta)
    r.update(dQ=dS @ k, dK=dS.transpose(-1, -2) @ q, dV=P.transpose(-1, -2) @ dO, dS=dS, delta=delta.squeeze(-1))
    if mags:
        r["A_dv"] = P.transpose(-1, -2) @ dO.abs()
        r["A_dq"] = dS.abs() @ k.abs()
        r["A_dk"] = dS.abs().transpose(-1, -2) @ q.abs()
        r["OdO"] = (dO.abs() * Ob.abs()).sum(-1)
        r["dOv"] = dO.abs() @ v.abs().transpose(-1, -2)
        r["D"] = (dP - delta).abs().masked_fill(~mask, 0.0)
    return r


def tables64(case: Case, device=None):
    """The fp32 rotary tables the kernels read, upcast: (n + 1, 64) float64 cos, sin."""
    cos, sin = rotary_tables(case.T, case.S, 64)
    return cos.double().to(device), sin.double().to(device)


def rope_fwd_ref(qkv, case: Case):
    """qkv float64 (B, n, 3*H*64) -> q (pre-scaled), k, v float64 in storage layout, padding rows zero."""
    cos, sin = tables64(case, qkv.device)
    outs = []
    for t, x in enumerate(qkv.chunk(3, dim=-1)):
        y = apply_rotary(tokens_to_heads(x, case.H), cos[:case.n], sin[:case.n])
        outs.append(pack(y * (QSCALE if t == 0 else 1.0), case))
    return outs


def rope_bwd_ref(dq, dk, dv, case: Case):
    """storage-layout float64 gradients -> dqkv (B, n, 3*H*64): the rotary inverse, q's third times qscale."""
    cos, sin = tables64(case, dq.device)
    parts = []
    for t, g in enumerate((dq, dk, dv)):
        x = unpack(g, case) * (QSCALE if t == 0 else 1.0)
        parts.append(heads_to_tokens(apply_rotary_inverse(x, cos[:case.n], sin[:case.n])))
    return torch.cat(parts, dim=-1)


def rotate_bound(e, case: Case):
    """A per-element error bound e (storage layout) of dq / dk / dv carried through the rotary inverse:
    |c| e + |s| e_partner per pair, token-major (B, n, H*64)."""
    cos, sin = tables64(case, e.device)
    x = unpack(e, case)
    return heads_to_tokens(apply_rotary_inverse(x, cos[:case.n].abs(), sin[:case.n].abs()))


# ---------------------------------------------------------------------------------------------------------------
# inputs
def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.bfloat16).double()


def _finish(case: Case, q, k, v, dO, probes=None):
    """(B, H, n, 64) float64 -> bf16-valued float64 storage tensors: Q / dO padding rows zero, K / V padding rows
    POISON (the planted key on the dropped last token's row is kept)."""
    d = {"q": pack(bf16_round(q), case), "k": pack(bf16_round(k), case, POISON), "v": pack(bf16_round(v), case, POISON),
         "dO": pack(bf16_round(dO), case), "probes": probes or []}
    return d


def _slice_scale(case: Case):
    return (1.0 + 0.25 * torch.arange(case.BH, dtype=torch.float64)).view(case.B, case.H, 1, 1)


def make_random(case: Case, seed: int = 0):
    """(a) N(0, 1.5) inputs (q pre-scaled by 1/8); slice (b, h) is scaled by 1 + 0.25 (b H + h) and its V offset by
    2 (b H + h), so a result read from the wrong slice is far outside every bound. dO is scaled like the inputs."""
    g = torch.Generator().manual_seed(seed)
    shp = (case.B, case.H, case.n, 64)
    sc = _slice_scale(case)
    q, k, v, dO = (torch.randn(shp, generator=g, dtype=torch.float64) * 1.5 * sc for _ in range(4))
    v = v + 2.0 * torch.arange(case.BH, dtype=torch.float64).view(case.B, case.H, 1, 1)
    return _finish(case, q * QSCALE, k, v, dO)


PROBES_PER_EDGE = 8
PLANT_SCORE = 10.0   # q_i . k_j of a planted forbidden key (allowed keys: |s| of a few units at most)
PLANT_BIAS = 12.0    # every query has q[63] = 1, a planted key k[63] = -PLANT_BIAS: low for every query but its own
PLANT_V = 8.0        # the planted key's value, in every dim (allowed keys' values are N(0, 1))
PLANT_DO = 8.0       # |dO| of a probe query, in every dim


def planted_key(qi: torch.Tensor) -> torch.Tensor:
    """The key aligned with query qi (..., 64) in dims 0..62 so that qi . k = PLANT_SCORE, dim 63 = -PLANT_BIAS."""
    a = qi.clone()
    a[..., 63] = 0.0
    kj = (PLANT_SCORE + PLANT_BIAS * qi[..., 63:64]) * a / (a * a).sum(-1, keepdim=True)
    kj[..., 63] = -PLANT_BIAS
    return kj


def edges(case: Case):
    """{edge name: [(query position i, forbidden key position j)]}: j lies directly across an edge of i's mask.
    Positions are sequence positions; j == n is the dropped last image token (its storage row exists)."""
    T, S, n, K, at = case.T, case.S, case.n, case.K, case.attn_type
    img = lambda r, c: T + r * S + c  # noqa: E731
    out = {"text_causal": [(i, i + 1) for i in range(T)]}   # i = T-1: the first image token across the text edge
    if at == "full":
        out["image_causal"] = [(i, i + 1) for i in range(T, n)]
    cells = [(r, c) for r in range(S) for c in range(S) if img(r, c) < n]
    if at == "axial_row":
        out["row_above_same_col"] = [(img(r, c), img(r - 1, c)) for r, c in cells if r >= 1]
        out["same_row_next_col"] = [(img(r, c), img(r, c + 1)) for r, c in cells if c + 1 < S]
    if at == "axial_col":
        out["col_left_same_row"] = [(img(r, c), img(r, c - 1)) for r, c in cells if c >= 1]
        out["same_col_next_row"] = [(img(r, c), img(r + 1, c)) for r, c in cells if r + 1 < S]
    if at == "conv_like":
        out["conv_left"] = [(img(r, c), img(r, c - K)) for r, c in cells if c - K >= 0]
        out["conv_up"] = [(img(r, c), img(r - K, c)) for r, c in cells if r - K >= 0]
        out["conv_corner"] = [(img(r, c), img(r - K, c - K)) for r, c in cells if r - K >= 0 and c - K >= 0]
        out["conv_up_right"] = [(img(r, c), img(r - 1, c + 1)) for r, c in cells if r >= 1 and c + 1 < S]
    return {k: v for k, v in out.items() if v}


def pad_probe_rows(case: Case):
    """The text / pad boundary: storage rows T .. Tp-1 hold no position; the planted inputs put aligned keys there
    for image (and late text) queries. Returns those storage rows."""
    return list(range(case.T, case.Tp))


def choose_probes(case: Case):
    """At least PROBES_PER_EDGE probes per edge (all of them where an edge has fewer candidates), no forbidden key
    used twice. First two queries of each preferred kind -- lane 0 and lane 31 of their 32-row storage tile, the
    first / last image row, the first / last image column -- then an even spread. Returns [(edge, i, j)]."""
    T, S = case.T, case.S
    st = storage_index(case.geom, case.attn_type)

    def kinds(i):
        lane = int(st[i]) % 32
        out = [f"lane{lane}"] if lane in (0, 31) else []
        if i >= T:
            r, c = divmod(i - T, S)
            out += [f"row{r}"] * (r in (0, S - 1)) + [f"col{c}"] * (c in (0, S - 1))
        return out

    used, probes = set(), []
    for name, cand in sorted(edges(case).items(), key=lambda kv: len(kv[1])):   # the scarcest edge chooses first
        cand = [ij for ij in cand if ij[1] not in used]
        pick, keys = [], set()

        def take(ij):
            if ij[1] not in keys:
                keys.add(ij[1])
                pick.append(ij)

        groups = {}
        for ij in cand:
            for kind in kinds(ij[0]):
                groups.setdefault(kind, []).append(ij)
        for kind in sorted(groups):
            for ij in (groups[kind][0], groups[kind][-1]):
                take(ij)
        want = max(PROBES_PER_EDGE, len(pick))
        step = max(1, len(cand) // (want + 1))
        for ij in cand[step // 2::step] + cand:   # an even spread, then (an edge with few candidates) what there is
            if len(pick) >= want:
                break
            take(ij)
        for i, j in pick:
            used.add(j)
            probes.append((name, i, j))
    return probes


def make_planted(case: Case, seed: int = 0):
    """(b) Small random inputs with, for every probe (i, j) of ``choose_probes``, the forbidden key j planted:
    k_j = ``planted_key(q_i)`` (score PLANT_SCORE, several units above anything allowed; a negative score for most
    other queries, so probes do not see each other's planted keys), v_j = PLANT_V, and
    dO_i = +-PLANT_DO. The text padding rows T .. Tp-1 get keys aligned with image / last-text queries and
    v = PLANT_V in place of the constant poison. ``probes``: [(edge, query storage row, key storage row)]."""
    g = torch.Generator().manual_seed(1000 + seed)
    shp = (case.B, case.H, case.n + 1, 64)   # position n: the dropped last image token's storage row
    q = torch.randn(shp, generator=g, dtype=torch.float64) * QSCALE
    q[..., 63] = 1.0
    k = torch.randn(shp, generator=g, dtype=torch.float64) * 0.5
    v = torch.randn(shp, generator=g, dtype=torch.float64)
    dO = torch.randn(shp, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand((64,), generator=g) < 0.5, -1.0, 1.0).double()
    probes = choose_probes(case)
    for _, i, j in probes:
        k[:, :, j] = planted_key(q[:, :, i])
        v[:, :, j] = PLANT_V
        dO[:, :, i] = PLANT_DO * sign
    d = _finish(case, q[:, :, :case.n], k[:, :, :case.n], v[:, :, :case.n], dO[:, :, :case.n])
    st = storage_index(case.geom, case.attn_type)
    last = int(st[case.n])
    d["k"][:, last] = bf16_round(k[:, :, case.n]).reshape(case.BH, 64)
    d["v"][:, last] = bf16_round(v[:, :, case.n]).reshape(case.BH, 64)
    out = [(name, int(st[i]), int(st[j])) for name, i, j in probes]
    # text / pad boundary: pad row T + t is aligned with a query that would see it if the text mask were off by one
    # or more: image queries (round-robin over lanes 0 / 31 / first / last) and the last text query
    pads = pad_probe_rows(case)
    if pads:
        I = case.S * case.S
        qpos = [case.T, case.T - 1, case.T + 31, case.n - 1, case.T + I // 2]
        qpos = [p for p in dict.fromkeys(qpos) if 0 <= p < case.n]
        for t, srow in enumerate(pads):
            i = qpos[t % len(qpos)]
            qi = d["q"][:, int(st[i])]
            d["k"][:, srow] = bf16_round(planted_key(qi))
            d["v"][:, srow] = PLANT_V
            d["dO"][:, int(st[i])] = bf16_round(PLANT_DO * sign).expand(case.BH, 64)
            out.append(("text_pad", int(st[i]), srow))
    d["probes"] = out
    return d


RAMP_SLOW = 3.0    # log2 units per key tile: below the rescale threshold
RAMP_FAST = 12.0   # above it


def ramp_heads(case: Case):
    """log2 units per ramp level, per head: even heads slow, odd heads fast."""
    return [RAMP_FAST if h % 2 else RAMP_SLOW for h in range(case.H)]


def ramp_level(case: Case, fast: bool) -> torch.Tensor:
    """(n,) ramp level of every key by its storage tile. A query visits its text tiles in order, then its local image
    tiles (not contiguous with the text tiles for the local patterns), so the levels are made to rise over any such
    path. Fast: text tile t -> min(t, 4), image tile u -> 5 + u mod 3 (every query with two tiles sees a rise of at
    least one level; top level 7: |s| to about 60). Slow: min(tile, 2) -- two rises of one level, and no path can
    rise by the threshold even in total."""
    tile = seq_to_storage(case) // 32
    if not fast:
        return tile.clamp(max=2).double()
    nt = case.Tp // 32
    return torch.where(tile < nt, tile.clamp(max=4), 5 + (tile - nt) % 3).double()


def make_ramp(case: Case, seed: int = 0):
    """(c) Scores that rise with the key's storage tile: k_j = level(j) e + noise, q_i = a e + noise with e a unit
    vector and a = step ln 2, so a key tile one level up raises a query's running maximum by about ``step`` log2
    units: RAMP_SLOW (below the forward's rescale threshold) in the even heads, RAMP_FAST (above) in the odd ones."""
    g = torch.Generator().manual_seed(2000 + seed)
    shp = (case.B, case.H, case.n, 64)
    e = torch.randn((64,), generator=g, dtype=torch.float64)
    e = e / e.norm()
    q = torch.randn(shp, generator=g, dtype=torch.float64) * 0.1
    k = torch.randn(shp, generator=g, dtype=torch.float64) * 0.5
    k = k - (k @ e).unsqueeze(-1) * e   # key noise orthogonal to e: the level alone sets a tile's maximum
    v = torch.randn(shp, generator=g, dtype=torch.float64)
    dO = torch.randn(shp, generator=g, dtype=torch.float64)
    for h, step in enumerate(ramp_heads(case)):
        q[:, h] += step * math.log(2.0) * e
        k[:, h] += ramp_level(case, step == RAMP_FAST).view(1, case.n, 1) * e
    return _finish(case, q, k, v, dO)


def tile_running_max(scores_log2: torch.Tensor):
    """scores (..., Np) in log2 units with -inf on masked keys -> per 32-key tile maxima (..., Np / 32)."""
    shp = scores_log2.shape
    return scores_log2.reshape(*shp[:-1], shp[-1] // 32, 32).max(dim=-1).values


# ---------------------------------------------------------------------------------------------------------------
# bounds (derived in test_attention_kernels_gpu.py's docstring), from reference quantities only
U = 2.0 ** -24    # fp32 unit roundoff
TINY = 2.0 ** -126   # smallest normal fp32 / bf16: the MFMAs and conversions flush what is below it to zero
BF = 2.0 ** -8    # one rounding to bf16: 8 significant bits, round to nearest, so half an ulp is up to 2^-8 |x|


def measure_transcendental_constant(n: int = 1 << 16, seed: int = 0) -> float:
    """The softmax chain p = exp2(x) / sum exp2(x), lse = log2(sum), evaluated in fp32 and in float64 on the CPU,
    for x in [-126, 8] (the kernels' range: lazy rescale keeps x <= 8): max relative error of exp2 and of 1 / l, and
    absolute error of log2 relative to max(1, |log2|)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g, dtype=torch.float64) * 134.0 - 126.0).float()
    e32, e64 = torch.exp2(x).double(), torch.exp2(x.double())
    rel_exp = ((e32 - e64).abs() / e64).max().item()
    l = (torch.rand(n, generator=g, dtype=torch.float64) * 4096.0 + 0.5).float()
    rel_rcp = (((1.0 / l).double() - 1.0 / l.double()).abs() * l.double()).max().item()
    lg32, lg64 = torch.log2(l).double(), torch.log2(l.double())
    abs_log = ((lg32 - lg64).abs() / lg64.abs().clamp_min(1.0)).max().item()
    return max(rel_exp, rel_rcp, abs_log)


def measure_rotation_constant(case_T: int = 257, S: int = 32) -> float:
    """The in-kernel rotary angle of the one-workgroup backward (revolutions = pos * hi - rint + pos * lo in fp32,
    attention_fused.hip rot_cs) against the fp32 tables: max |cos - cos_table|, |sin - sin_table| with the last step
    (cos / sin of the fp32 revolutions) in float64."""
    from dalle_amd.models.rotary import IMAGE_TEXT_POS, TEXT_AXIAL_POS, rotary_freq_split

    rotf, n_lang, n_pix, _, _ = rotary_freq_split(64)
    hi, lo = rotf[:32], rotf[32:]
    cos, sin = rotary_tables(case_T, S, 64)
    n = case_T + S * S - 1
    p = torch.arange(n)
    kk = (p - case_T).clamp(min=0)
    inv = torch.tensor(2.0 / (S - 1), dtype=torch.float32)
    worst = 0.0
    for j in range(n_lang + 2 * n_pix):
        if j < n_lang:
            pos = torch.where(p < case_T, p.float(), torch.tensor(IMAGE_TEXT_POS))
        else:
            coord = (kk // S if j < n_lang + n_pix else kk % S).float()
            pos = torch.where(p < case_T, torch.tensor(TEXT_AXIAL_POS), -1.0 + inv * coord)
        r = pos * hi[j]
        r = r - torch.round(r)
        r = torch.addcmul(r, pos, lo[j])   # fp32 (one rounding more than the kernel's fma)
        ang = r.double() * 2.0 * math.pi
        worst = max(worst, (torch.cos(ang) - cos[:n, 2 * j].double()).abs().max().item(),
                    (torch.sin(ang) - sin[:n, 2 * j + 1].double()).abs().max().item())
    return worst


C_T_MEASURED = 6.61e-8          # measure_transcendental_constant(), pinned by test_attn_ref_cpu.py
C_T = 4 * C_T_MEASURED         # hardware exp2 / log2 / rcp
C_ROT_MEASURED = 1.66e-6       # measure_rotation_constant(), pinned by test_attn_ref_cpu.py
C_ROT = 4 * C_ROT_MEASURED     # in-kernel rotary angles + hardware sin / cos against the fp32 tables


def p_rel_error_fwd(r, case: Case):
    """(BH, Np) relative error of the forward's normalised P_ij before its bf16 rounding: twice the error of
    exp2 (numerator and row sum: 67 u smax on the exponent -- 64 fp32 accumulations of exact bf16 products, the
    LOG2E multiply, the fma, the stale-max product -- plus the hardware exp2), Np + 2 roundings of the row sum and
    its rescales, the hardware rcp."""
    eps = 67 * U * r["smax"] + C_T
    return 2 * eps + (case.Np + 2) * U + C_T


def fwd_bounds(r, case: Case):
    """-> (bound of out (BH, Np, 64), bound of lse (BH, Np))."""
    rho = p_rel_error_fwd(r, case).unsqueeze(-1)
    b_out = BF * r["O"].abs() + (1 + BF) * (BF + rho + case.Np * U) * r["A_o"]
    # an unnormalised p below TINY is flushed; the row sum is at least 2^-RESCALE_THR (stale maximum)
    b_out = b_out + TINY * (1.0 + 2.0 ** RESCALE_THR * r["vabs_sum"])
    eps = 67 * U * r["smax"] + C_T
    b_lse = LOG2E * (eps + case.Np * U + C_T) + 3 * U * (r["lse"].abs() + RESCALE_THR + math.log2(case.Np))
    return b_out, b_lse


def bwd_errors(r, q, k, v, dO, case: Case):
    """fp32 error of dq, dk, dv before the one bf16 output rounding, storage layout (BH, Np, 64) each."""
    # relative error of the backward's P_ij = exp2(s log2e - lse): the exponent, the fp32 lse it is given, exp2
    rho = (67 * U * r["smax"] + math.log(2.0) * U * r["lse"].abs() + C_T).unsqueeze(-1)      # (BH, Np, 1), per query
    P, dS = r["P"], r["dS"].abs()
    e_dv = P.transpose(-1, -2) @ ((BF + rho + case.Np * U) * dO.abs()) + TINY * dO.abs().sum(dim=1, keepdim=True)
    # |d dS_ij| <= (bf + rho_i) |dS_ij| + 65 u P_ij (sum_d |dO_id||v_jd| + sum_d |dO_id||O_id|)
    G = P * (r["dOv"] + r["OdO"].unsqueeze(-1))
    # a P_ij below TINY is flushed to zero and its dS_ij = P_ij (dP_ij - delta_i) is lost, as is a dS_ij below TINY
    E = (BF + rho + case.Np * U) * dS + 65 * U * G + TINY * (1.0 + r["D"])
    e_dq = E @ k.abs()
    e_dk = E.transpose(-1, -2) @ q.abs()
    return e_dq, e_dk, e_dv


def storage_bounds(r, errs):
    """attn_bwd's bf16 dq / dk / dv in storage layout."""
    return [BF * r[n].abs() + (1 + BF) * e + TINY for n, e in zip(("dQ", "dK", "dV"), errs)]


def dqkv_bound(dqkv_ref, r, errs, case: Case, in_kernel_angles: bool):
    """attn_bwd_rope's dqkv: the fp32 errors carried through the rotation (4 more fp32 roundings on the rotated
    magnitudes; C_ROT on the pair's unrotated magnitudes when the angles are computed in-kernel), then the one bf16
    rounding."""
    parts = []
    for t, (name, e) in enumerate(zip(("dQ", "dK", "dV"), errs)):
        sc = QSCALE if t == 0 else 1.0
        g = r[name].abs() * sc
        rot = rotate_bound(e * sc, case) + 4 * U * rotate_bound(g, case)
        if in_kernel_angles:   # an angle off by d moves cos by d |sin| and sin by d |cos|: both of the pair, unweighted
            gp = unpack(g, case)
            rot = rot + C_ROT * heads_to_tokens(gp + rotate_pairs(gp))
        parts.append(rot)
    e = torch.cat(parts, dim=-1)
    return BF * dqkv_ref.abs() + (1 + BF) * e + TINY


# ---------------------------------------------------------------------------------------------------------------
# the cases of test_attention_kernels_gpu.py (the planted ones are also checked for sensitivity on the CPU)
GEOMS = [(1, 8), (32, 8), (33, 16), (65, 16), (257, 32), (256, 32), (40, 64)]


def patterns_for(S: int):
    pats = [("full", 5), ("axial_row", 5), ("axial_col", 5), ("conv_like", 1), ("conv_like", 3), ("conv_like", 5)]
    return pats + ([("conv_like", 9)] if S == 8 else [])


def cases():
    """Every (T, S) x pattern; slices (B, H) = (2, 4) (B*H = 8: the XCD remap) for the axial patterns and conv_like
    K = 5, (1, 3) (no remap) for the rest, (1, 2) at S = 64, and (2, 8) (two remap rounds) once more at (65, 16)."""
    out = []
    for T, S in GEOMS:
        for at, K in patterns_for(S):
            if S == 64:
                B, H = 1, 2
            elif at in ("axial_row", "axial_col") or (at, K) == ("conv_like", 5):
                B, H = 2, 4
            else:
                B, H = 1, 3
            out.append(Case(T, S, at, K, B, H))
            if (T, S) == (65, 16) and K == 5:
                out.append(Case(T, S, at, K, 2, 8))
    return out


MAKERS = {"random": make_random, "planted": make_planted, "ramp": make_ramp}


def bundle(case: Case, kind: str, device=None, backward: bool = True):
    """Inputs, references and bounds of one case, computed once on ``device``; only (B*H, Np, 64)-sized tensors are
    kept. Keys: q k v dO (storage, float64), out_tok / dO_tok (token-major (B, n, H*64)), O lse b_out b_lse, and with
    ``backward``: lse32 (the fp32 lse the backward kernels are given), dQ dK dV + b_dq b_dk b_dv, dqkv +
    b_dqkv_tables / b_dqkv_angles, real, probes."""
    d = MAKERS[kind](case)
    probes = d.pop("probes")
    q, k, v, dO = (d[n].to(device) for n in ("q", "k", "v", "dO"))
    fwd = attention_ref(q, k, v, case)
    b_out, b_lse = fwd_bounds(fwd, case)
    out = {"q": q, "k": k, "v": v, "dO": dO, "O": fwd["O"], "lse": fwd["lse"], "b_out": b_out, "b_lse": b_lse,
           "real": fwd["real"], "probes": probes, "dO_tok": heads_to_tokens(unpack(dO, case))}
    if not backward:
        return out
    ob = bf16_round(fwd["O"]) * fwd["real"].view(1, -1, 1)
    del fwd
    r = attention_ref(q, k, v, case, dO=dO, out_bf16=ob)
    errs = bwd_errors(r, q, k, v, dO, case)
    b_dq, b_dk, b_dv = storage_bounds(r, errs)
    dqkv = rope_bwd_ref(r["dQ"], r["dK"], r["dV"], case)
    out.update(out_tok=heads_to_tokens(unpack(ob, case)), lse32=r["lse"].float(), dQ=r["dQ"], dK=r["dK"], dV=r["dV"],
               b_dq=b_dq, b_dk=b_dk, b_dv=b_dv, dqkv=dqkv, b_dqkv_tables=dqkv_bound(dqkv, r, errs, case, False),
               b_dqkv_angles=dqkv_bound(dqkv, r, errs, case, True))
    return out
