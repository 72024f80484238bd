"""Autoregressive text->image decoding with a KV cache (BASELINE config 5).

One decode step pushes ONE position through every layer: fused LayerNorm + cached token shift
(per-branch LN history), QKV GEMM, rotary into the KV cache, sparse decode attention over only the
keys the layer's static pattern allows (text prefix + row / column / 5x5 window), output GEMM,
LayerScale residual, then the final norm, the image-vocabulary head and sampling (temperature,
top-k, top-p, Gumbel-max). Every positional quantity is read from a device scalar, so on MI355X the
whole step is captured ONCE into a hipGraph and replayed for each of the 1024 image tokens.

The CPU path runs the same step with the reference ops (tests compare it against the full forward).
"""
from __future__ import annotations

import contextlib
import gc
import math
import os
import threading
import weakref
from typing import List, Optional

import torch
import torch.nn.functional as F

from .patterns import PATTERN_IDS, static_mask
from .rotary import apply_rotary, rotary_tables

# hipGraph captures of different engines (e.g. one serving generator per GPU, each in its own thread)
# run one at a time, in thread-local capture mode: another thread's replays and allocations on its own
# device neither break a capture nor are refused while it runs
_CAPTURE_LOCK = threading.Lock()


@contextlib.contextmanager
def _capture_into(graph):
    """Capture the body into ``graph`` (one capture at a time, thread-local mode). Dead Python cycles are collected
    first and the collector is paused until the capture ends: torch collects before a capture only on request, and a
    cycle that dies inside one while it holds another engine's captured graph releases that graph's memory pool from
    the capturing thread, which the runtime refuses during a capture -- in a destructor, so the process aborts."""
    with _CAPTURE_LOCK:
        gc.collect()
        paused = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                yield
        finally:
            if paused:
                gc.enable()


def filter_logits(logits: torch.Tensor, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """K18: top-k then nucleus filtering (fill -inf); graph-capturable (no host sync)."""
    if top_k and top_k > 0:
        kth = torch.topk(logits, min(top_k, logits.shape[-1]), dim=-1).values[..., -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p is not None and top_p < 1.0:
        sorted_logits, sorted_idx = torch.sort(logits, descending=True, dim=-1)
        cum = torch.softmax(sorted_logits, dim=-1).cumsum(-1)
        remove = cum - torch.softmax(sorted_logits, dim=-1) > top_p  # keep the token that crosses top_p
        sorted_logits = sorted_logits.masked_fill(remove, float("-inf"))
        logits = torch.full_like(logits, float("-inf")).scatter(-1, sorted_idx, sorted_logits)
    return logits


def gumbel_sample(logits: torch.Tensor, temperature: float = 1.0, generator=None) -> torch.Tensor:
    u = torch.rand(logits.shape, device=logits.device, generator=generator).clamp_(1e-20, 1.0)
    return torch.argmax(logits / max(temperature, 1e-10) - torch.log(-torch.log(u)), dim=-1)


def _guidance_scale(guided: bool, cond_scale: Optional[float]) -> Optional[float]:
    """The ``cond_scale`` argument of a ``generate`` call, checked: the scale a guided engine's captured step
    reads (default 1), None for a plain engine (which takes no scale)."""
    if not guided:
        if cond_scale is not None:
            raise ValueError("cond_scale needs an engine built with guided=True")
        return None
    s = 1.0 if cond_scale is None else float(cond_scale)
    if s < 0:
        raise ValueError(f"cond_scale must be >= 0, got {s}")
    return s


def filter_logits_rows(logits: torch.Tensor, top_k_rows: torch.Tensor, top_p_rows: torch.Tensor) -> torch.Tensor:
    """``filter_logits`` with one ``(top_k, top_p)`` pair per row of ``logits`` (rows, V), vectorised over the rows:
    row ``r`` of the result is ``filter_logits(logits[r], top_k_rows[r], top_p_rows[r])`` (``top_k <= 0`` or ``>= V``
    and ``top_p >= 1`` switch the respective filter off for that row)."""
    V = logits.shape[-1]
    k = top_k_rows.to(logits.device, torch.long).view(-1, 1)
    p = top_p_rows.to(logits.device, logits.dtype).view(-1, 1)
    kth = torch.sort(logits, descending=True, dim=-1).values.gather(-1, k.clamp(1, V) - 1)  # the k-th largest, per row
    logits = logits.masked_fill((k > 0) & (logits < kth), float("-inf"))
    sorted_logits, sorted_idx = torch.sort(logits, descending=True, dim=-1)
    probs = torch.softmax(sorted_logits, dim=-1)
    remove = (probs.cumsum(-1) - probs > p) & (p < 1.0)  # keep the token that crosses top_p
    sorted_logits = sorted_logits.masked_fill(remove, float("-inf"))
    return torch.full_like(logits, float("-inf")).scatter(-1, sorted_idx, sorted_logits)


def _is_rows(x) -> bool:
    """A per-picture sequence (list, tuple, array, tensor of one or more dimensions), as opposed to a scalar."""
    if isinstance(x, torch.Tensor):
        return x.dim() > 0
    return isinstance(x, (list, tuple)) or (hasattr(x, "__len__") and not isinstance(x, (str, bytes)))


def _scalars_only(**params):
    """A plain engine's sampling arguments, checked: per-picture sequences need a row-parameter engine."""
    for name, x in params.items():
        if _is_rows(x):
            raise ValueError(f"{name} is a per-picture sequence: that needs an engine built with row_params=True")
    if params.get("noise_row") is not None:
        raise ValueError("noise_row needs an engine built with row_params=True")


def row_generator_seed(seed: int, noise_row: int) -> int:
    """The torch step's noise of a row-parameter engine: row ``r`` draws from its own ``torch.Generator``, seeded at the
    start of ``generate`` with ``(seed[r] * 2**24 + noise_row[r]) mod 2**63`` -- a function of the row's own two table
    entries only, so its draws depend neither on its slot nor on its neighbours."""
    return (int(seed) * (1 << 24) + int(noise_row)) % (1 << 63)


def _row_tables(batch: int, guided: bool, temperature, top_k, top_p, seed, cond_scale, noise_row) -> dict:
    """The sampling arguments of a row-parameter ``generate`` call, checked on the host and broadcast: CPU tensors of
    ``batch`` entries each -- temperature fp32, top_k int32, top_p fp32, seed int64, noise_row int32 (default
    ``arange``) and, guided, cond_scale fp32. Each argument is a scalar or holds ``batch`` entries."""
    def row(x, name, default, conv):
        if x is None:
            x = default
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().tolist()
        elif _is_rows(x):
            x = [v.item() if isinstance(v, torch.Tensor) else v for v in x]
        if not isinstance(x, list):
            x = [x] * batch
        if len(x) != batch:
            raise ValueError(f"{name} must be a scalar or hold one entry per picture ({batch}), got {len(x)}")
        return [conv(v) for v in x]

    if not guided and cond_scale is not None:
        raise ValueError("cond_scale needs an engine built with guided=True")
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    t = {"temperature": row(temperature, "temperature", 1.0, float),
         "top_k": row(top_k, "top_k", 0, lambda v: min(max(int(v or 0), 0), 2 ** 31 - 1)),
         "top_p": row(top_p, "top_p", 1.0, lambda v: 1.0 if v is None else float(v)),
         "seed": row(seed, "seed", 0, int),
         "noise_row": row(noise_row, "noise_row", list(range(batch)), int)}
    if guided:
        t["cond_scale"] = row(cond_scale, "cond_scale", 1.0, float)
        for s in t["cond_scale"]:
            if not s >= 0:
                raise ValueError(f"cond_scale must be >= 0, got {s}")
    for p in t["top_p"]:
        if not math.isfinite(p):
            raise ValueError(f"top_p must be finite, got {p}")
    for s in t["seed"]:
        if not -(2 ** 63) <= s < 2 ** 63:
            raise ValueError(f"seed must fit 64 bits, got {s}")
    for r in t["noise_row"]:
        if not 0 <= r < 2 ** 24:
            raise ValueError(f"noise_row must lie in [0, 2**24), got {r}")
    dt = {"temperature": torch.float32, "top_k": torch.int32, "top_p": torch.float32, "seed": torch.int64,
          "noise_row": torch.int32, "cond_scale": torch.float32}
    return {k: torch.tensor(v, dtype=dt[k]) for k, v in t.items()}


def _check_inpaint(image, regen, batch: int, L: int, prime=None):
    """The ``image`` / ``regen`` arguments of a ``generate`` call, checked: (batch, L) integer codes and a
    (batch, L) bool mask (True = regenerate), both or neither, and not together with ``prime``."""
    if image is None and regen is None:
        return False
    if image is None or regen is None:
        raise ValueError("image and regen go together: the picture's codes and the mask of positions to regenerate")
    if prime is not None:
        raise ValueError("give either prime (a forced prefix) or image + regen (a mask), not both")
    for name, t in (("image", image), ("regen", regen)):
        if t.dim() != 2 or t.shape[0] != batch or t.shape[1] != L:
            raise ValueError(f"{name} must be (batch {batch}, {L}), got {tuple(t.shape)}")
    if image.dtype.is_floating_point or image.dtype == torch.bool:
        raise ValueError("image must hold integer image codes")
    if regen.dtype != torch.bool:
        raise ValueError("regen must be a bool mask (True = regenerate)")
    return True


def _regen_window(regen: torch.Tensor):
    """(k0, last): the smallest and the largest position any row regenerates (one host read); (L, -1) when no row
    regenerates anything."""
    L = regen.shape[1]
    col = regen.any(0)
    idx = torch.arange(L, device=regen.device)
    k0, last = torch.stack([torch.where(col, idx, L).min(), torch.where(col, idx, -1).max()]).tolist()
    return int(k0), int(last)


class DecodeEngine:
    def __init__(self, model, batch_size: int, device=None, use_hip: Optional[bool] = None, skinny: bool = True,
                 partials: int = 2, fused_sampler: bool = True, guided: bool = False, row_params: bool = False):
        """``row_params``: per-picture sampling parameters. The engine then owns device tables of one temperature,
        top-k, top-p, seed, noise row and (guided) guidance scale per picture, which its step always reads in place of
        the scalars: ``generate`` takes a scalar or a sequence for each, and one captured graph serves every setting.
        ``guided``: classifier-free guidance. The engine then owns ``2 * batch_size`` rows -- the pictures' captions
        on top, the null caption below -- and samples picture ``r`` from ``u + cond_scale * (c - u)`` of rows ``r`` /
        ``r + batch_size`` (in the fused sampler's one launch), feeding the chosen code back to both rows.
        ``skinny``: decode projections on the skinny MFMA GEMM with fused epilogues (when the shapes allow);
        ``partials``: 2 = every projection leaves split-K slabs summed by its consumer (measured fastest,
        profiles/r2_decode_partials_ab.txt), 1 = the residual projections only, 0 = in-GEMM split-K hand-off
        (the non-default forms are kept for the numerics A/B in tests/test_generation_gpu.py);
        ``fused_sampler``: the one-kernel top-k / top-p / Gumbel sampler (K18)."""
        self.model = model
        cfg = self.cfg = model.cfg
        self.B = batch_size  # pictures, as callers see it; R rows of caches, histories and buffers
        self.guided = bool(guided)
        self.R = 2 * batch_size if self.guided else batch_size
        self.device = device or next(model.parameters()).device
        dev = self.device
        if use_hip is None:
            from ..ops.ext import hip_available
            use_hip = dev.type == "cuda" and hip_available()
        self.use_hip = use_hip
        self.T, self.S, self.n = cfg.text_len, cfg.image_fmap_size, cfg.seq_len
        self.H, self.Dh, self.d = cfg.heads, cfg.dim_head, cfg.dim
        self.Vt = cfg.total_text_tokens
        self.cdt = torch.bfloat16 if use_hip else torch.float32
        tr = model.transformer
        self.pairs = tr.layers.pairs()
        self.geom = tr.geom
        L, B = len(self.pairs), self.R
        self.kc = [torch.zeros(B * self.H, self.n, self.Dh, dtype=self.cdt, device=dev) for _ in range(L)]
        self.vc = [torch.zeros_like(k) for k in self.kc]
        self.hist = [[torch.zeros(B, self.n, self.d, dtype=self.cdt, device=dev) for _ in range(2)] for _ in range(L)]
        self.cos, self.sin = rotary_tables(self.T, self.S, self.Dh, device=dev)
        self.pos = torch.zeros((), dtype=torch.int32, device=dev)
        # 1 while every row carries the same caption (set per generate call, on device: a captured graph serves both
        # cases): the decode attention then reads the text positions' K / V from row 0's cache for all rows
        self.text_shared = torch.zeros(1, dtype=torch.int32, device=dev)
        self.share_text = True
        # guided: the per-row form of the same saving. Row r reads the text positions' K / V from row text_src[r]'s
        # cache: the null rows from the first null row, the caption rows from row 0 when all captions are equal,
        # else from themselves (filled per generate call, on device). ``share_src`` = False: every row its own.
        # An engine with ``text_src`` set passes it to the decode attention in place of ``text_shared``.
        self.text_src = torch.arange(B, dtype=torch.int32, device=dev) if self.guided else None
        self.share_src = True
        self.cond_scale = torch.ones(1, dtype=torch.float32, device=dev) if self.guided else None
        self._null_text = None
        self.tok = torch.zeros(B, dtype=torch.long, device=dev)
        self.hbuf = torch.zeros(B, self.d, dtype=self.cdt, device=dev)
        self.qbuf = torch.zeros(B, self.H, self.Dh, dtype=self.cdt, device=dev)
        self.obuf = torch.zeros(B, self.H * self.Dh, dtype=self.cdt, device=dev)
        self.codes = torch.zeros(B, cfg.image_seq_len, dtype=torch.long, device=dev)
        self.temperature, self.top_k, self.top_p = 1.0, 0, 1.0
        # fused HIP sampler (K18); its Gumbel noise is a counter hash of (seed, position, row, token)
        self.fused_sampler = use_hip and fused_sampler
        self.seed = torch.zeros((), dtype=torch.int64, device=dev)
        # forced prefix (image-primed generation): image positions [0, n_prime) take prime's code instead of the
        # sample. Both live on the device, so one captured graph serves every prefix length, 0 included
        self.prime = torch.zeros(B, cfg.image_seq_len, dtype=torch.long, device=dev)
        self.n_prime = torch.zeros((), dtype=torch.int32, device=dev)
        # inpainting: per picture, the positions that take prime's code as well (1 = keep); all zero otherwise. The
        # captured step always reads it, so the same graph serves unprimed, prefix and masked calls
        self.keep = torch.zeros(batch_size, cfg.image_seq_len, dtype=torch.uint8, device=dev)
        self.row_params = bool(row_params)
        if self.row_params:
            n = batch_size
            self.row_temperature = torch.ones(n, dtype=torch.float32, device=dev)
            self.row_top_k = torch.zeros(n, dtype=torch.int32, device=dev)
            self.row_top_p = torch.ones(n, dtype=torch.float32, device=dev)
            self.row_seed = torch.zeros(n, dtype=torch.int64, device=dev)
            self.noise_row = torch.arange(n, dtype=torch.int32, device=dev)
            self.row_cond_scale = torch.ones(n, dtype=torch.float32, device=dev) if self.guided else None
            self._row_gens = None  # the torch step's per-row generators (seeded per generate call)
        self.graph = None
        self._pf_graphs = {}  # captured caption prefills, by (rows, input buffer)
        self._pf_masks = {}   # contiguous (P, P) caption blocks of the layer patterns
        self._static_logits = None
        self._w = {}
        # decode-step projections through the skinny MFMA GEMM (csrc/kernels/skinny.hip) with the
        # rotary / GEGLU / LayerScale-residual epilogues fused: M = batch <= 64 rows
        self.skinny = (use_hip and skinny and B <= 64 and self.d % 128 == 0 and (cfg.ff_mult * self.d) % 128 == 0)
        self.sk_cnt = torch.zeros(8192, dtype=torch.int32, device=dev) if self.skinny else None
        # split-K partials: the projections leave fp32 slabs summed by their consumer, so those GEMMs
        # split K over 4-8x the workgroups with no cross-workgroup hand-off. 2 (default): out-proj /
        # FF-out slabs summed by the next LayerNorm, QKV slabs by the attention prologue (under the KV
        # stream); 1: residual projections only; 0: in-GEMM split-K hand-off
        # (profiles/r2_decode_partials_ab.txt: 4.02 -> 3.70-3.73 ms per image-position step)
        mode = int(partials) if self.skinny else 0
        self.partials = mode in (1, 2)
        self.qkv_partials = mode == 2
        # pending residual update of a stream, not yet applied: (stream, slabs, bias, LayerScale) or None
        self._pending = None

    # -- weights (one bf16 cast per generate call) --------------------------------------------------
    def _wt(self, p):
        ent = self._w.get(id(p))
        if ent is None:
            ent = (p, p.detach().to(self.cdt))
            self._w[id(p)] = ent
        return ent[1]

    _refresh_weights = True

    def reset(self):
        """Zero position/caches and refresh the compute-dtype weight copies IN PLACE (a captured graph
        keeps pointing at the same buffers, so weight updates between calls are still seen)."""
        self.pos.zero_()
        self.n_prime.zero_()
        self.keep.zero_()
        if self._refresh_weights:
            for p, w in self._w.values():
                w.copy_(p.detach().reshape(w.shape))
        for k in self.kc + self.vc:
            k.zero_()

    # -- branch steps -------------------------------------------------------------------------------
    def _flush_pending(self):
        if self._pending is not None:
            from ..ops.hip_ops import C
            C().residual_from_partials_(*self._pending)
            self._pending = None

    def _ln_shift(self, ls, hist, x):
        pre = ls.fn
        if self.use_hip:
            from ..ops.hip_ops import C
            if self._pending is not None and self._pending[0] is not x:  # another stream's update: apply it now
                self._flush_pending()
            part, pbias, pscale = self._pending[1:] if self._pending is not None else (None, None, None)
            self._pending = None
            C().decode_ln_shift_(x, pre.norm.weight.detach(), pre.norm.bias.detach(), hist, self.hbuf, self.pos,
                                 self.T, self.S, bool(pre.fn.enabled), part, pbias, pscale)
            return self.hbuf
        y = F.layer_norm(x, (self.d,), pre.norm.weight, pre.norm.bias)
        p = int(self.pos)
        hist[:, p] = y
        if not pre.fn.enabled:
            return y
        out = y.clone()
        q, h2 = self.d // 4, self.d // 2
        if p < self.T:
            out[:, :h2] = hist[:, p - 1, :h2] if p >= 1 else 0.0
        else:
            k = p - self.T
            out[:, :q] = hist[:, p - self.S, :q] if k >= self.S else 0.0
            out[:, q:h2] = hist[:, p - 1, q:h2] if k % self.S else 0.0
        return out

    def _attn_res(self, li, ls, x_in, x_res):
        """x_res += LayerScale * Attention(LN-shift(x_in)); one skinny GEMM each for QKV (+rotary into
        the KV cache) and the output projection (+bias, LayerScale, residual) on the fused path."""
        if not self.skinny:
            return self._residual(x_res, self._attn(li, ls, x_in), ls)
        from ..ops.hip_ops import C
        attn = ls.fn.fn.fn
        h = self._ln_shift(ls, self.hist[li][0], x_in)
        if self.qkv_partials:
            part = C().skinny_partials(h, self._wt(attn.to_qkv.weight))
            C().decode_attn_part_(part, self.cos, self.sin, self.Dh ** -0.5, self.kc[li], self.vc[li], self.obuf, self.pos,
                                  self.T, self.S, self.H, self.geom.kernel_size, PATTERN_IDS[attn.attn_type], **self._text_kw())
        else:
            C().skinny_qkv_rope_(h, self._wt(attn.to_qkv.weight), self.cos, self.sin, self.qbuf, self.kc[li], self.vc[li],
                                 self.pos, self.H, self.Dh ** -0.5, self.sk_cnt)
            C().decode_attn_(self.qbuf, self.kc[li], self.vc[li], self.obuf, self.pos, self.T, self.S, self.H,
                             self.geom.kernel_size, PATTERN_IDS[attn.attn_type], **self._text_kw())
        if self.partials:
            po = C().skinny_partials(self.obuf, self._wt(attn.to_out[0].weight))
            self._pending = (x_res, po, self._wt(attn.to_out[0].bias), self._scale(ls))
            return x_res
        C().skinny_residual_(x_res, self.obuf, self._wt(attn.to_out[0].weight), self._wt(attn.to_out[0].bias),
                             self._scale(ls), self.sk_cnt)
        return x_res

    def _ff_res(self, li, ls, x_in, x_res):
        """x_res += LayerScale * FF(LN-shift(x_in)): FF1 with GEGLU and FF2 with the residual fused."""
        if not self.skinny:
            return self._residual(x_res, self._ff(li, ls, x_in), ls)
        from ..ops.hip_ops import C
        ff = ls.fn.fn.fn
        h = self._ln_shift(ls, self.hist[li][1], x_in)
        a = C().skinny_geglu(h, self._wt(ff.net[0].weight), self._wt(ff.net[0].bias), self.sk_cnt)
        if self.partials:
            self._pending = (x_res, C().skinny_partials(a, self._wt(ff.net[3].weight)), self._wt(ff.net[3].bias),
                             self._scale(ls))
            return x_res
        C().skinny_residual_(x_res, a, self._wt(ff.net[3].weight), self._wt(ff.net[3].bias), self._scale(ls), self.sk_cnt)
        return x_res

    def _text_kw(self):
        """Where the decode attention reads the text positions' K / V: the all-rows flag, or the per-row sources."""
        return {"text_shared": self.text_shared} if self.text_src is None else {"text_src": self.text_src}

    def _scale(self, ls):
        ent = self._w.get(("scale", id(ls.scale)))
        if ent is None:
            ent = (ls.scale, ls.scale.detach().reshape(-1).float().contiguous())
            self._w[("scale", id(ls.scale))] = ent
        return ent[1]

    def _attn(self, li, ls, x):
        attn = ls.fn.fn.fn
        h = self._ln_shift(ls, self.hist[li][0], x)
        qkv = F.linear(h, self._wt(attn.to_qkv.weight))
        if self.use_hip:
            from ..ops.hip_ops import C
            C().decode_rope_(qkv.contiguous(), self.cos, self.sin, self.qbuf, self.kc[li], self.vc[li], self.pos, self.H,
                             self.Dh ** -0.5)
            C().decode_attn_(self.qbuf, self.kc[li], self.vc[li], self.obuf, self.pos, self.T, self.S, self.H,
                             self.geom.kernel_size, PATTERN_IDS[attn.attn_type], **self._text_kw())
            o = self.obuf
        else:
            o = self._attn_torch(li, attn, qkv)
        return F.linear(o, self._wt(attn.to_out[0].weight), self._wt(attn.to_out[0].bias))

    def _attn_torch(self, li, attn, qkv):
        from ..ops.reference import split_heads
        from .rotary import apply_rotary
        p = int(self.pos)
        B, H, Dh = self.R, self.H, self.Dh
        q, k, v = (t.view(B, H, 1, Dh) for t in qkv.chunk(3, dim=-1))
        c, s = self.cos[p:p + 1], self.sin[p:p + 1]
        q, k, v = (apply_rotary(t, c, s) for t in (q, k, v))
        kc = self.kc[li].view(B, H, self.n, Dh)
        vc = self.vc[li].view(B, H, self.n, Dh)
        kc[:, :, p] = k[:, :, 0]
        vc[:, :, p] = v[:, :, 0]
        mask = static_mask(self.geom, attn.attn_type, self.n, device=q.device)[p, : p + 1]
        sc = (q * Dh ** -0.5) @ kc[:, :, : p + 1].transpose(-1, -2)
        sc = sc.masked_fill(~mask, float("-inf"))
        o = torch.softmax(sc, -1) @ vc[:, :, : p + 1]
        return o.reshape(B, H * Dh)

    def _ff(self, li, ls, x):
        ff = ls.fn.fn.fn
        h = self._ln_shift(ls, self.hist[li][1], x)
        a = F.linear(h, self._wt(ff.net[0].weight), self._wt(ff.net[0].bias))
        if self.use_hip:
            from ..ops.hip_ops import C
            a = C().geglu_fwd(a.contiguous())
        else:
            a1, g = a.chunk(2, -1)
            a = a1 * F.gelu(g)
        return F.linear(a, self._wt(ff.net[3].weight), self._wt(ff.net[3].bias))

    def _residual(self, x, y, ls):
        """x += LayerScale * y (fp32 residual stream), one fused kernel on the HIP path."""
        if self.use_hip:
            from ..ops.hip_ops import C
            C().scale_residual_(x, y.contiguous(), ls.scale.detach().reshape(-1).contiguous())
            return x
        return x + y.float() * ls.scale.detach().view(1, -1)

    # -- one position through the whole network ------------------------------------------------------
    def _forward_position(self) -> torch.Tensor:
        W = self.model.to_logits[1].weight
        x = F.embedding(self.tok, W.detach()).float()
        self._pending = None
        if self.cfg.reversible:
            x1, x2 = x, x.clone()
            for li, (f, g) in enumerate(self.pairs):
                x1 = self._attn_res(li, f, x2, x1)
                x2 = self._ff_res(li, g, x1, x2)
            self._flush_pending()
            out = (x1 + x2) * 0.5
        else:
            for li, (f, g) in enumerate(self.pairs):
                x = self._attn_res(li, f, x, x)
                x = self._ff_res(li, g, x, x)
            self._flush_pending()
            out = x
        norm, head = self.model.to_logits[0], self.model.to_logits[1]
        h = F.layer_norm(out, (self.d,), norm.weight.detach(), norm.bias.detach())
        if self.skinny:
            from ..ops.hip_ops import C
            return C().skinny_linear(h.to(self.cdt), self._wt(head.weight)[self.Vt:], self._wt(head.bias)[self.Vt:], True,
                                     self.sk_cnt)
        return F.linear(h.to(self.cdt), self._wt(head.weight)[self.Vt:], self._wt(head.bias)[self.Vt:]).float()

    def _step(self):
        """Graph body for ANY position: run position ``pos``; choose the next input token on device --
        the next caption token while ``pos + 1 < T`` (prefill), else the sampled image token -- and
        record the sample as image code ``pos - T + 1`` (prefill writes are overwritten later)."""
        if self.row_params:
            return self._step_rows()
        logits = self._forward_position()
        if self.fused_sampler and logits.dtype == torch.float32 and logits.shape[-1] <= 8192:
            # one HIP launch (csrc/kernels/sample.hip): filter + sample + codes / next-token bookkeeping
            from ..ops.hip_ops import C
            C().sample_step(logits, int(self.top_k or 0), float(1.0 if self.top_p is None else self.top_p),
                            float(self.temperature), self.seed, self.pos, self.text_bos, self.codes, self.tok, self.Vt,
                            prime=self.prime, n_prime=self.n_prime, keep=self.keep,
                            **({"cond_scale": self.cond_scale} if self.guided else {}))
            self.pos.add_(1)
            return logits
        B, R = self.B, self.R
        if self.guided:  # the sampler's mix: three separately rounded fp32 operations
            c, u = logits[:B].float(), logits[B:].float()
            logits = u + self.cond_scale * (c - u)
        logits = filter_logits(logits, self.top_k, self.top_p)
        nxt = gumbel_sample(logits, self.temperature)
        p = self.pos.long()
        ci = p - (self.T - 1)
        idx = ci.clamp(0, self.cfg.image_seq_len - 1).view(1, 1).expand(B, 1)
        forced = (ci < self.n_prime) | (self.keep.gather(1, idx).view(B) != 0)
        nxt = torch.where((ci >= 0) & (ci < self.cfg.image_seq_len) & forced, self.prime[:B].gather(1, idx).view(B), nxt)
        if self.guided:  # both halves take the picture's code
            nxt = torch.cat([nxt, nxt])
            idx = idx.repeat(2, 1)
        self.codes.scatter_(1, idx, nxt.view(R, 1))
        nxt_text = self.text_bos.gather(1, (p + 1).clamp(max=self.T - 1).view(1, 1).expand(R, 1)).view(R)
        self.tok.copy_(torch.where(p + 1 < self.T, nxt_text, nxt + self.Vt))
        self.pos.add_(1)
        return logits

    def _step_rows(self):
        """``_step`` of a row-parameter engine: the same step, every sampling scalar read from the per-picture tables."""
        logits = self._forward_position()
        if self.fused_sampler and logits.dtype == torch.float32 and logits.shape[-1] <= 8192:
            from ..ops.hip_ops import C
            C().sample_step(logits, 0, 1.0, 1.0, self.seed, self.pos, self.text_bos, self.codes, self.tok, self.Vt,
                            prime=self.prime, n_prime=self.n_prime, keep=self.keep,
                            row_temperature=self.row_temperature, row_top_k=self.row_top_k, row_top_p=self.row_top_p,
                            row_seed=self.row_seed, noise_row=self.noise_row,
                            **({"cond_scale": self.cond_scale, "row_cond_scale": self.row_cond_scale} if self.guided else {}))
            self.pos.add_(1)
            return logits
        B = self.B
        if self.guided:  # the sampler's mix, with the picture's own scale
            c, u = logits[:B].float(), logits[B:].float()
            logits = u + self.row_cond_scale.view(B, 1) * (c - u)
        logits = filter_logits_rows(logits.float(), self.row_top_k, self.row_top_p)
        # row r's uniforms from its own generator (``row_generator_seed``); greedy where the temperature is <= 1e-10
        u = torch.stack([torch.rand(logits.shape[-1], generator=g) for g in self._row_gens]).clamp_(1e-20, 1.0).to(logits.device)
        t = self.row_temperature.view(B, 1)
        greedy = ~(t > 1e-10)
        noisy = logits / torch.where(greedy, torch.ones_like(t), t) - torch.log(-torch.log(u))
        nxt = torch.argmax(torch.where(greedy, logits, noisy), dim=-1)
        self._book(nxt)
        return logits

    def _book(self, nxt: torch.Tensor):
        """The torch step's bookkeeping for the (B,) samples: forced codes, ``codes``, the next input token, ``pos``."""
        B, R = self.B, self.R
        p = self.pos.long()
        ci = p - (self.T - 1)
        idx = ci.clamp(0, self.cfg.image_seq_len - 1).view(1, 1).expand(B, 1)
        forced = (ci < self.n_prime) | (self.keep.gather(1, idx).view(B) != 0)
        nxt = torch.where((ci >= 0) & (ci < self.cfg.image_seq_len) & forced, self.prime[:B].gather(1, idx).view(B), nxt)
        if self.guided:  # both halves take the picture's code
            nxt = torch.cat([nxt, nxt])
            idx = idx.repeat(2, 1)
        self.codes.scatter_(1, idx, nxt.view(R, 1))
        nxt_text = self.text_bos.gather(1, (p + 1).clamp(max=self.T - 1).view(1, 1).expand(R, 1)).view(R)
        self.tok.copy_(torch.where(p + 1 < self.T, nxt_text, nxt + self.Vt))
        self.pos.add_(1)

    _image_step = _step

    def _set_rows(self, tables: dict, lo: int = 0):
        """Load this engine's pictures' entries ``[lo, lo + B)`` of the checked tables (``_row_tables``)."""
        hi = lo + self.B
        self.row_temperature.copy_(tables["temperature"][lo:hi])
        self.row_top_k.copy_(tables["top_k"][lo:hi])
        self.row_top_p.copy_(tables["top_p"][lo:hi])
        self.row_seed.copy_(tables["seed"][lo:hi])
        self.noise_row.copy_(tables["noise_row"][lo:hi])
        if self.guided:
            self.row_cond_scale.copy_(tables["cond_scale"][lo:hi])
        self._row_gens = [torch.Generator().manual_seed(row_generator_seed(s, r))
                          for s, r in zip(tables["seed"][lo:hi].tolist(), tables["noise_row"][lo:hi].tolist())]
        self.temperature, self.top_k, self.top_p = 1.0, 0, 1.0  # the scalars are not read
        self.seed.zero_()

    # -- public API ---------------------------------------------------------------------------------
    def _rows_text(self, text_bos: torch.Tensor) -> torch.Tensor:
        """The caption table of all rows: a guided engine puts the null caption (``prepare_text`` of pad ids) under
        the caller's (B, T) captions; a table that already holds 2 B rows passes."""
        if not self.guided or text_bos.shape[0] == self.R:
            return text_bos
        if self._null_text is None:
            zeros = torch.zeros(1, self.cfg.text_seq_len, dtype=text_bos.dtype, device=text_bos.device)
            self._null_text = self.model.prepare_text(zeros)
        return torch.cat([text_bos, self._null_text.to(text_bos.dtype).expand(self.B, -1)])

    def _start(self, text_bos: torch.Tensor):
        self.reset()
        text_bos = self._rows_text(text_bos)
        if not hasattr(self, "text_bos") or self.text_bos.shape != text_bos.shape:
            self.text_bos = torch.zeros_like(text_bos)
        self.text_bos.copy_(text_bos)
        self.tok.copy_(text_bos[:, 0])
        if self.guided:
            # text_shared: all CAPTION rows equal (the null rows always are). Sources: caption rows -> row 0 if so,
            # else themselves; null rows -> the first null row
            B = self.B
            self.text_shared.copy_((text_bos[:B] == text_bos[:1]).all().view(1))
            if self.share_src:
                self.text_src[:B].copy_(torch.arange(B, dtype=torch.int32, device=self.device) * (1 - self.text_shared))
                self.text_src[B:].fill_(B)
            else:
                self.text_src.copy_(torch.arange(self.R, dtype=torch.int32, device=self.device))
        elif self.share_text:
            self.text_shared.copy_((text_bos == text_bos[:1]).all().view(1))
        else:
            self.text_shared.zero_()

    def set_prime(self, prime: Optional[torch.Tensor]):
        """Force the first ``k`` image tokens of the steps that follow to ``prime`` (B, k), 0 <= k < image_seq_len
        (None: no prefix). ``reset`` clears the count, so this goes after the last reset of a call."""
        if prime is None:
            self.n_prime.zero_()
            self.keep.zero_()
            return
        L = self.cfg.image_seq_len
        if prime.dim() != 2 or prime.shape[0] != self.B or not 0 <= prime.shape[1] < L:  # B pictures: the sampler reads rows [0, B)
            raise ValueError(f"prime must be (batch {self.B}, k) with 0 <= k < {L}, got {tuple(prime.shape)}")
        if prime.dtype.is_floating_point or prime.dtype == torch.bool:
            raise ValueError("prime must hold integer image codes")
        k = prime.shape[1]
        if k:
            self.prime[:self.B, :k].copy_(prime)
        self.n_prime.fill_(k)

    def set_keep(self, image: torch.Tensor, regen: torch.Tensor):
        """Inpainting: the steps that follow keep ``image``'s code (B, image_seq_len) wherever ``regen`` (same shape,
        bool) is False and sample the rest. Like ``set_prime``, it goes after the last reset of a call."""
        _check_inpaint(image, regen, self.B, self.cfg.image_seq_len)
        self.prime[:self.B].copy_(image)
        self.keep.copy_(~regen)

    def _warm_weights(self):
        """Create the compute-dtype copies of every weight the prefill and the decode steps read, on the current
        stream (a split engine calls this before its part streams fork: the parts share the copies, and a copy made
        on one part's stream would be read by the other's without an ordering)."""
        for f, g in self.pairs:
            attn, ff = f.fn.fn.fn, g.fn.fn.fn
            for p in (attn.to_qkv.weight, attn.to_out[0].weight, attn.to_out[0].bias, ff.net[0].weight, ff.net[0].bias,
                      ff.net[3].weight, ff.net[3].bias):
                self._wt(p)
            self._scale(f)
            self._scale(g)

    @torch.no_grad()
    def prefill(self, text_bos: torch.Tensor):
        """Eagerly feed BOS + text positions 0..T-2 (position T-1 is the first sampling step)."""
        self._start(text_bos)
        text_bos = self.text_bos  # all rows' captions (a guided engine added the null rows)
        for p in range(self.T - 1):
            self.tok.copy_(text_bos[:, p])
            self._forward_position()
            self.pos.add_(1)
        self.tok.copy_(text_bos[:, self.T - 1])

    # -- parallel prefill: the caption positions as ONE batched pass per layer -------------------------
    def _pf_ln_shift(self, ls, hist, x):
        """LN + cached token shift over all prefill positions at once: fills hist[:, :P] and returns the
        shifted rows (the text shift takes channels [0, d/2) from the previous position; rows past the caption,
        a pass that runs on over kept image codes, take the image shift of ``_ln_shift``: channels [0, d/4) from the
        cell above, [d/4, d/2) from the cell to the left)."""
        pre = ls.fn
        P, T, S = x.shape[1], self.T, self.S
        if self.use_hip and self.d in (256, 512, 1024, 2048):  # one kernel: LN, history rows, pushed shift
            from ..ops.hip_ops import C
            out = torch.empty(x.shape, dtype=self.cdt, device=x.device)
            C().prefill_ln_shift_(x, pre.norm.weight.detach(), pre.norm.bias.detach(), hist, out, bool(pre.fn.enabled),
                                  float(pre.norm.eps), T, S)
            return out
        y = F.layer_norm(x, (self.d,), pre.norm.weight.detach(), pre.norm.bias.detach(), pre.norm.eps).to(self.cdt)
        hist[:, :P] = y
        if not pre.fn.enabled:
            return y
        out = y.clone()
        q, h2 = self.d // 4, self.d // 2
        Tt = min(T, P)
        out[:, 1:Tt, :h2] = y[:, :Tt - 1, :h2]
        out[:, 0, :h2] = 0
        if P > T:  # image rows k = p - T
            out[:, T:, :h2] = 0
            if P > T + S:
                out[:, T + S:, :q] = y[:, T:P - S, :q]
            left = (torch.arange(P - T, device=x.device) % S != 0).view(1, -1, 1)
            out[:, T:, q:h2] = torch.where(left, y[:, T - 1:P - 1, q:h2], torch.zeros((), dtype=y.dtype, device=x.device))
        return out

    def _pf_attn(self, li, ls, x):
        attn = ls.fn.fn.fn
        B, P, H, Dh = x.shape[0], x.shape[1], self.H, self.Dh
        h = self._pf_ln_shift(ls, self.hist[li][0][:B], x)
        kc, vc = self.kc[li][: B * H], self.vc[li][: B * H]  # the first B rows' caches (all of them, or row 0)
        if self.use_hip:
            # the projections on the assembly GEMM where the rows tile (_pf_linear); one kernel rotates q / k / v and
            # writes k / v into the caches (q pre-scaled, bf16 as in the decode steps); scores in fp32, then one
            # masked-softmax kernel to bf16 probabilities. Returns the bf16 projection output (bias included).
            from ..ops.hip_ops import C
            qkv = self._pf_linear(h.view(B * P, self.d), attn.to_qkv.weight).view(B, P, -1)
            q = torch.empty(B * H, P, Dh, dtype=self.cdt, device=x.device)
            C().prefill_rope_(qkv, self.cos, self.sin, q, kc, vc, H, Dh ** -0.5)
            k, v = kc[:, :P], vc[:, :P]
            if P <= min(self.T - 1, 512):  # the caption: one (P, P) block, a row's scores in registers (8 per lane)
                sc = torch.bmm(q, k.transpose(1, 2), out_dtype=torch.float32)
                pr = torch.empty(sc.shape, dtype=self.cdt, device=x.device)
                C().prefill_softmax_(sc, self._pf_mask(attn.attn_type, P, x.device), pr)
                o = torch.bmm(pr, v)
            else:
                # past the caption (kept image codes): blocks of queries against the keys up to the block's last
                # (the rest is causally masked), so the fp32 scores stay at (rows, block, keys); each block reads its
                # rows of the layer's whole static mask
                mask = static_mask(self.geom, attn.attn_type, self.n, device=x.device)
                Qb = P if P <= self.pf_dense_max else self.pf_query_block
                o = torch.empty(B * H, P, Dh, dtype=self.cdt, device=x.device)
                for q0 in range(0, P, Qb):
                    Q = min(Qb, P - q0)
                    Pk = q0 + Q
                    sc = torch.bmm(q[:, q0:Pk], kc[:, :Pk].transpose(1, 2), out_dtype=torch.float32)
                    pr = torch.empty(sc.shape, dtype=self.cdt, device=x.device)
                    C().prefill_softmax_block_(sc, mask, pr, q0)
                    torch.bmm(pr, vc[:, :Pk], out=o[:, q0:Pk])
            o = o.view(B, H, P, Dh).transpose(1, 2).reshape(B * P, H * Dh)
            return self._pf_linear(o, attn.to_out[0].weight, attn.to_out[0].bias).view(B, P, -1)
        qkv = F.linear(h, self._wt(attn.to_qkv.weight)).view(B, P, 3, H, Dh).permute(2, 0, 3, 1, 4).float()
        c, sn = self.cos[:P], self.sin[:P]
        q, k, v = (apply_rotary(t, c, sn) for t in qkv)
        kc.view(B, H, self.n, Dh)[:, :, :P] = k.to(self.cdt)
        vc.view(B, H, self.n, Dh)[:, :, :P] = v.to(self.cdt)
        # the cached (rounded) keys / values, as the decode steps will read them
        k, v = k.to(self.cdt).float(), v.to(self.cdt).float()
        sc = (q * Dh ** -0.5) @ k.transpose(-1, -2)
        mask = static_mask(self.geom, attn.attn_type, self.n, device=x.device)[:P, :P]
        o = torch.softmax(sc.masked_fill(~mask, float("-inf")), -1) @ v
        o = o.transpose(1, 2).reshape(B, P, H * Dh).to(self.cdt)
        return F.linear(o, self._wt(attn.to_out[0].weight), self._wt(attn.to_out[0].bias))

    def _pf_linear(self, x2, w, b=None):
        """x2 (M, K) bf16 . W^T (+ b) for the prefill: the assembly GEMM where the rows tile (its epilogue reads the
        fp32 bias parameter), else hipBLASLt -- with the engine's own bf16 copies either way, never the per-forward
        cast cache (a captured prefill must hold only buffers that outlive it)."""
        from ..ops.hip_ops import ASM_GEMM, C, _asm_ok
        wb = self._wt(w)
        if ASM_GEMM and _asm_ok(x2, wb) and (b is None or (b.dtype == torch.float32 and b.is_contiguous())):
            return C().asm_gemm(x2, wb, None if b is None else b.detach(), None)
        return F.linear(x2, wb, None if b is None else self._wt(b))

    def _pf_mask(self, attn_type: str, P: int, device):
        """The layer pattern's (P, P) caption block, contiguous (cached: the first, eager prefill fills it before
        the pass is captured)."""
        key = (attn_type, P)
        m = self._pf_masks.get(key)
        if m is None:
            m = static_mask(self.geom, attn_type, self.n, device=device)[:P, :P].contiguous()
            self._pf_masks[key] = m
        return m

    def _pf_ff(self, li, ls, x):
        ff = ls.fn.fn.fn
        B, P = x.shape[0], x.shape[1]
        h = self._pf_ln_shift(ls, self.hist[li][1][:B], x)
        if self.use_hip:
            from ..ops.hip_ops import C
            u = C().geglu_fwd(self._pf_linear(h.view(B * P, self.d), ff.net[0].weight, ff.net[0].bias))
            return self._pf_linear(u, ff.net[3].weight, ff.net[3].bias).view(B, P, -1)
        a = F.linear(h, self._wt(ff.net[0].weight), self._wt(ff.net[0].bias))
        val, gate = a.float().chunk(2, -1)
        u = (val * F.gelu(gate)).to(self.cdt)
        return F.linear(u, self._wt(ff.net[3].weight), self._wt(ff.net[3].bias))

    def _pf_add(self, x, ls, y):
        """x + LayerScale * y for a sublayer's projection output y: in place, one kernel, on MI355X."""
        if self.use_hip and self.d % 4 == 0:
            from ..ops.hip_ops import C
            C().prefill_residual_(x, y, self._scale(ls))
            return x
        return x + y.float() * self._scale(ls)

    def _pf_rows(self) -> int:
        """Rows the caption prefill runs for (after ``_start``): 1 when every row holds row 0's caption (a
        host read of the device flag: the one synchronisation of the prefill), else the batch."""
        if self.guided:
            # all rows, whatever the sources (no host read): the prefill's library GEMMs pick their algorithm by
            # the row count, so a pass over the source rows' prefix [0, B] rounds differently from the full pass
            # and guided sampling would depend, in the last bit, on whether the text reads are shared. The pass is
            # under 2 % of a call; the saving of sharing is in the 1024 decode steps' reads
            return self.R
        one = self.use_hip and self.share_text and self.B > 1 and bool(self.text_shared.item())
        return 1 if one else self.B

    pf_dense_max = 512    # a prefill of up to this many positions takes its scores in one block
    pf_query_block = 256  # queries per score block of a longer one (tests lower both to run the blocks on a small model)

    @torch.no_grad()
    def prefill_parallel(self, text_bos: torch.Tensor, rows: Optional[int] = None, started: bool = False,
                         kept: Optional[torch.Tensor] = None):
        """Positions 0..T-2 (BOS + caption) as one batched pass per layer instead of T-1 decode steps:
        fills the KV caches and LN histories exactly where the steps would, then leaves the engine at
        position T-1 (the first sampling step) -- at batch 64 on the reference model this replaces
        ~0.9 s of sequential steps with a few ms.

        One caption repeated over the batch (the decode attention then reads the text keys / values from row
        0's cache, ``text_shared``): the pass runs for row 0 alone, and the other rows get only what the decode
        steps read of their own: the LN history at position T-2 (the shift of the first step, at T-1).
        ``rows`` / ``started``: given by a caller that already ran ``_start`` and ``_pf_rows`` (a split
        engine, which then launches the parts' passes on their streams with no host read in between).

        ``kept`` (B, k0) image codes, k0 >= 1: the pass runs on over the picture's first ``k0`` codes, which every row
        keeps (inpainting) -- P = T - 1 + k0 positions, inputs the caption then codes 0 .. k0 - 2 -- and leaves the
        engine at position P with code k0 - 1 as the next input, so the first decode step samples code k0. It
        runs for all rows (the image keys / values are per row; the decode steps' shared text reads stay as they
        are) and eagerly: a captured graph per distinct k0 would each hold a private pool."""
        if not started:
            self._start(text_bos)
        if kept is not None and kept.shape[1] > 0:
            k0 = kept.shape[1]
            if kept.shape[0] != self.R:  # guided: both halves are fed the pictures' codes
                kept = kept.repeat(self.R // kept.shape[0], 1)
            kept = kept.to(self.text_bos.dtype) + self.Vt
            P = self.T - 1 + k0
            self._pf_body(self.R, P, torch.cat([self.text_bos, kept[:, :k0 - 1]], dim=1))
            self.pos.fill_(P)
            self.tok.copy_(kept[:, k0 - 1])
            self.codes[:, :k0].copy_(kept - self.Vt)
            return
        P = self.T - 1
        if rows is None:
            rows = self._pf_rows()
        if P > 0:
            if self.use_hip:
                # the pass is ~25 launches per layer: captured once per (rows, input buffer) and replayed
                key = (rows, self.text_bos.data_ptr())
                graph = self._pf_graphs.get(key)
                if graph is None:
                    self._pf_body(rows, P)  # the result, and the libraries' warm-up for the capture
                    graph = torch.cuda.CUDAGraph()
                    with _capture_into(graph):
                        self._pf_body(rows, P)
                    self._pf_graphs[key] = graph
                else:
                    graph.replay()
            else:
                self._pf_body(rows, P)
            self.pos.fill_(P)
        self.tok.copy_(self.text_bos[:, P])

    def _pf_body(self, rows: int, P: int, tokens: Optional[torch.Tensor] = None):
        """``tokens`` (rows, P): the input ids of the P positions (default: the caption)."""
        W = self.model.to_logits[1].weight.detach()
        x = F.embedding(self.text_bos[:rows, :P] if tokens is None else tokens, W).float()
        if self.cfg.reversible:
            x1, x2 = x, x.clone()
            for li, (f, g) in enumerate(self.pairs):
                x1 = self._pf_add(x1, f, self._pf_attn(li, f, x2))
                x2 = self._pf_add(x2, g, self._pf_ff(li, g, x1))
        else:
            for li, (f, g) in enumerate(self.pairs):
                x = self._pf_add(x, f, self._pf_attn(li, f, x))
                x = self._pf_add(x, g, self._pf_ff(li, g, x))
        if rows < self.R:  # the other rows' own reads: the LN history the first decode step shifts in
            for hs in self.hist:
                for hb in hs:
                    hb[rows:, P - 1].copy_(hb[0, P - 1].expand(self.B - rows, -1))

    @torch.no_grad()
    def generate(self, text_bos: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 use_graph: Optional[bool] = None, seed: Optional[int] = None, parallel_prefill: Optional[bool] = None,
                 prime: Optional[torch.Tensor] = None, cond_scale: Optional[float] = None,
                 image: Optional[torch.Tensor] = None, regen: Optional[torch.Tensor] = None, prefill_kept: bool = True,
                 skip_tail: bool = True, noise_row=None) -> torch.Tensor:
        """The caption prefill (one batched pass per layer, ``parallel_prefill``, default on; else T-1
        decode steps) then the 1024 sampled image tokens through one step function; on MI355X that step
        is a single hipGraph replayed per position. ``seed`` fixes the fused sampler's noise (default:
        drawn from torch's global generator). ``prime`` (B, k) image codes: the first ``k`` image tokens are
        forced to them (ordinary decode steps whose sample is replaced) and the rest sampled; the noise stays a
        function of (seed, position, row, token), so positions >= k draw what an unprimed call draws there.
        ``cond_scale`` (guided engines only): the guidance scale, a device scalar the captured step reads -- another
        scale replays the same graph; 1 samples from the conditional rows' logits, 0 from the null caption's.
        ``image`` (B, image_seq_len) codes with ``regen`` (same shape, bool): inpainting. Every position is still
        sampled given the caption and all earlier positions, but where ``regen`` is False the picture's code is kept
        in place of the sample (per row; an all-True row is an ordinary unprimed row). Two savings, both on by
        default: ``prefill_kept`` -- the codes before the first regenerated position of any row go through the
        batched prefill together with the caption, not through decode steps; ``skip_tail`` -- no steps run after the
        last regenerated position of any row. The noise of a regenerated position is the unmasked call's.
        On a ``row_params`` engine ``temperature``, ``top_k``, ``top_p``, ``seed`` and (guided) ``cond_scale`` each take
        a scalar or one entry per picture, and ``noise_row`` (default ``arange(B)``) names the row of each picture's
        noise key: picture ``j`` samples with its own entries, its noise a function of (seed[j], position,
        noise_row[j], token) -- not of its slot. All are checked on the host before anything is launched."""
        masked = _check_inpaint(image, regen, self.B, self.cfg.image_seq_len, prime)
        tables = None
        if self.row_params:
            tables = _row_tables(self.B, self.guided, temperature, top_k, top_p, seed, cond_scale, noise_row)
            temperature, top_k, top_p, seed, cond_scale = 1.0, 0, 1.0, 0, None
            if use_graph and not self.fused_sampler:
                raise ValueError("the torch sampling step of a row-parameter engine draws from host generators: no graph")
            if use_graph is None:
                use_graph = self.use_hip and self.fused_sampler
        else:
            _scalars_only(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, cond_scale=cond_scale,
                          noise_row=noise_row)
        s = _guidance_scale(self.guided, cond_scale)
        if s is not None:
            self.cond_scale.fill_(s)
        k0, last = 0, self.cfg.image_seq_len - 1
        if masked:
            image, regen = image.to(self.device, torch.long), regen.to(self.device)
            w0, w1 = _regen_window(regen)
            if w1 < 0:  # nothing to regenerate
                return image.clone()
            k0, last = (w0 if prefill_kept else 0), (w1 if skip_tail else last)
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.seed.fill_(int(seed))
        if tables is not None:
            self._set_rows(tables)
        use_graph = self.use_hip if use_graph is None else use_graph
        if parallel_prefill is None:
            parallel_prefill = True
        self._start(text_bos)
        if use_graph:
            self._capture()
        if parallel_prefill:
            self.prefill_parallel(text_bos, kept=image[:, :k0] if k0 else None)
            first = self.T - 1 + k0
        else:
            self._start(text_bos)
            first = 0
        # after the last reset (``_start`` above, or the one inside ``prefill_parallel``)
        if masked:
            self.set_keep(image, regen)
        else:
            self.set_prime(prime)
        for _ in range(self.T + last - first):  # positions first .. T - 1 + last
            if use_graph:
                self.graph.replay()
            else:
                self._step()
        if last + 1 < self.cfg.image_seq_len:  # the kept tail: no step ran for it
            self.codes[:, last + 1:].copy_(image[:, last + 1:].repeat(self.R // self.B, 1))  # guided: both halves
        return self.codes[:self.B].clone()

    def _capture(self):
        """Capture one image step into a hipGraph (warm-up on a side stream as torch requires)."""
        if self.graph is not None and (self.row_params or self._graph_cfg == (self.temperature, self.top_k, self.top_p)):
            return  # row parameters live in device tables: one capture serves every later call
        # warm-up on a side stream (allocator / library handles), then capture; the caller resets the
        # state (pos, tokens, caches) afterwards, so the warm-up steps leave no trace
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with _capture_into(g):
            self._static_logits = self._step()
        self.graph = g
        self._graph_cfg = (self.temperature, self.top_k, self.top_p)

    @torch.no_grad()
    def teacher_forced_logits(self, text_bos: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        """Image-vocab logits at every position >= T-1 when feeding the given image codes (tests)."""
        self.prefill(text_bos)
        if image.shape[0] != self.R:  # guided: both halves are fed the pictures' codes
            image = image.repeat(self.R // image.shape[0], 1)
        outs = []
        for i in range(self.cfg.image_seq_len):
            outs.append(self._forward_position())
            if i + 1 < self.cfg.image_seq_len:
                self.tok.copy_(image[:, i] + self.Vt)
                self.pos.add_(1)
        return torch.stack(outs, dim=1)


class _PartGraphs:
    """One image-position step of every part: each part's own captured graph replayed on the part's stream
    (the ``graph`` of a :class:`SplitDecodeEngine`)."""

    def __init__(self, eng):
        self.eng = weakref.ref(eng)  # not a cycle: a dropped engine frees its graphs at once, not in a later collection

    def replay(self):
        self.eng().replay_steps(1)


class SplitDecodeEngine:
    """The batch split into ``parts`` independent :class:`DecodeEngine` s whose steps run concurrently
    on separate HIP streams. At batch 64 a decode step is a chain of short kernels whose time is mostly
    fixed latency (a skinny GEMM takes 8-10 us whether it streams 2 or 16 MB of weights), so two
    half-batch chains interleaved on the GPU overlap one chain's latency with the other's work. The
    parts share the bf16 weight copies; each has its own KV caches, LN histories, device position and
    sampler seed (``seed + part``), so the parts never touch the same buffer.

    Each part's step is captured as its own LINEAR graph, replayed on the part's stream with no per-step join:
    the HIP runtime launches a linear graph from pre-built packets, 0.17 ms of host time per step for both
    parts. (One graph with the parts as parallel branches is launched node by node, ~2.5 ms of host time per
    ~3 ms step: profiles/r6_decode_replay_host.txt, 3.00-3.02 vs 3.05-3.11 ms per step.)"""

    def __init__(self, model, batch_size: int, device=None, parts: int = 2, guided: bool = False,
                 row_params: bool = False):
        """``row_params``: every part is a row-parameter engine and takes its slice of the caller's tables as they are
        (no part index is added to the seeds: the table is the truth).
        ``guided``: every part is a guided engine over its slice of the pictures, with its own conditional and
        null rows, so no part reads another's buffers."""
        if batch_size % parts:
            raise ValueError(f"batch {batch_size} is not divisible into {parts} parts")
        self.model, self.B, self.nparts = model, batch_size, parts
        self.guided = bool(guided)
        self.row_params = bool(row_params)
        kw = {"row_params": True} if self.row_params else {}
        self.parts = [DecodeEngine(model, batch_size // parts, device=device, guided=guided, **kw) for _ in range(parts)]
        for p in self.parts[1:]:
            p._w = self.parts[0]._w  # one bf16 copy of every weight, refreshed by part 0 only
            p._refresh_weights = False
        self.device = self.parts[0].device
        self.use_hip = self.parts[0].use_hip
        self.graph = None
        self._graph_cfg = None
        self._part_streams = None

    @property
    def codes(self) -> torch.Tensor:
        return torch.cat([p.codes[:p.B] for p in self.parts])

    def _start_all(self, text_bos: torch.Tensor):
        b = self.B // self.nparts
        for i, p in enumerate(self.parts):
            p._start(text_bos[i * b:(i + 1) * b])

    _start = _start_all

    def _step(self):
        for p in self.parts:
            p._step()

    _image_step = _step

    @torch.no_grad()
    def prefill(self, text_bos: torch.Tensor):
        b = self.B // self.nparts
        for i, p in enumerate(self.parts):
            p.prefill(text_bos[i * b:(i + 1) * b])

    @torch.no_grad()
    def prefill_parallel(self, text_bos: torch.Tensor, kept: Optional[torch.Tensor] = None):
        """Every part's caption prefill, the parts' passes concurrently on the part streams (with distinct
        captions each pass is ~0.7 ms of mid-size GEMMs per layer for 32 rows: run one after the other
        they took 93 ms per generate call). The shared-caption flags are read on the host first, so no
        synchronisation falls between the launches. ``kept`` (B, k0): the passes run on over the pictures' first
        k0 codes (``DecodeEngine.prefill_parallel``), each part over its rows of them."""
        b = self.B // self.nparts
        slices = [text_bos[i * b:(i + 1) * b] for i in range(self.nparts)]
        kepts = [None if kept is None else kept[i * b:(i + 1) * b] for i in range(self.nparts)]
        for p, t in zip(self.parts, slices):
            p._start(t)
        rows = [p._pf_rows() for p in self.parts]
        if not self.use_hip:
            for p, t, r, kp in zip(self.parts, slices, rows, kepts):
                p.prefill_parallel(t, rows=r, started=True, kept=kp)
            return
        if self._part_streams is None:
            self._part_streams = [torch.cuda.Stream() for _ in self.parts]
        if kept is not None or self.row_params:
            # an eager pass creates the shared bf16 weight copies where it first needs them: make them here, on the
            # main stream, so that no part reads a copy another part's stream is still writing
            self.parts[0]._warm_weights()
        main = torch.cuda.current_stream()
        for st in self._part_streams:
            st.wait_stream(main)
        for p, t, r, kp, st in zip(self.parts, slices, rows, kepts, self._part_streams):
            with torch.cuda.stream(st):
                p.prefill_parallel(t, rows=r, started=True, kept=kp)
        for st in self._part_streams:
            main.wait_stream(st)

    def _capture(self):
        # a row-parameter engine's capture is keyed on nothing: its parts read every setting from their tables
        cfg = None if self.row_params else (self.parts[0].temperature, self.parts[0].top_k, self.parts[0].top_p)
        if self.graph is not None and self._graph_cfg == cfg:
            return
        for p in self.parts:
            p._capture()  # a linear graph of the part's own step (its warm-up steps are reset by the prefill)
        if self._part_streams is None:
            self._part_streams = [torch.cuda.Stream() for _ in self.parts]
        self.graph = _PartGraphs(self)
        self._graph_cfg = cfg

    @torch.no_grad()
    def generate(self, text_bos: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 use_graph: Optional[bool] = None, seed: Optional[int] = None,
                 prime: Optional[torch.Tensor] = None, cond_scale: Optional[float] = None,
                 image: Optional[torch.Tensor] = None, regen: Optional[torch.Tensor] = None, prefill_kept: bool = True,
                 skip_tail: bool = True, noise_row=None) -> torch.Tensor:
        """``DecodeEngine.generate`` over the parts. ``image`` / ``regen`` (inpainting) are sliced per part; the
        prefill over kept codes and the step window use the bounds over ALL rows, so the parts stay in step. With
        ``row_params`` every per-picture table (``noise_row`` included, default ``arange(B)`` over the whole batch) is
        sliced per part as given."""
        tables = None
        if self.row_params:
            tables = _row_tables(self.B, self.guided, temperature, top_k, top_p, seed, cond_scale, noise_row)
            temperature, top_k, top_p, seed, cond_scale = 1.0, 0, 1.0, 0, None
        else:
            _scalars_only(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, cond_scale=cond_scale,
                          noise_row=noise_row)
        if prime is not None and (prime.dim() != 2 or prime.shape[0] != self.B):
            raise ValueError(f"prime must be (batch {self.B}, k), got {tuple(prime.shape)}")
        L = self.parts[0].cfg.image_seq_len
        masked = _check_inpaint(image, regen, self.B, L, prime)
        k0, last = 0, L - 1
        if masked:
            image, regen = image.to(self.device, torch.long), regen.to(self.device)
            w0, w1 = _regen_window(regen)
            if w1 < 0:  # nothing to regenerate
                return image.clone()
            k0, last = (w0 if prefill_kept else 0), (w1 if skip_tail else last)
        s = _guidance_scale(self.guided, cond_scale)
        if s is not None:
            for p in self.parts:
                p.cond_scale.fill_(s)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        for i, p in enumerate(self.parts):
            p.temperature, p.top_k, p.top_p = temperature, top_k, top_p
            p.seed.fill_(int(seed) + i)
            if tables is not None:
                p._set_rows(tables, i * p.B)
        use_graph = self.use_hip if use_graph is None else use_graph
        self._start_all(text_bos)
        if use_graph:
            self._capture()
        self.prefill_parallel(text_bos, kept=image[:, :k0] if k0 else None)
        b = self.B // self.nparts
        for i, p in enumerate(self.parts):  # after the parts' last reset (inside ``prefill_parallel``)
            if masked:
                p.set_keep(image[i * b:(i + 1) * b], regen[i * b:(i + 1) * b])
            else:
                p.set_prime(None if prime is None else prime[i * b:(i + 1) * b])
        steps = last - k0 + 1  # image positions k0 .. last
        if use_graph:
            self.replay_steps(steps)
        else:
            for _ in range(steps):
                for p in self.parts:
                    p._step()
        if last + 1 < L:  # the kept tail: no step ran for it
            for i, p in enumerate(self.parts):
                p.codes[:, last + 1:].copy_(image[i * b:(i + 1) * b, last + 1:].repeat(p.R // p.B, 1))
        return self.codes.clone()

    def replay_steps(self, k: int):
        """``k`` decode steps through the captured graphs: the part streams fork from the current stream, each
        replays its part's graph ``k`` times with no join in between, and the current stream joins them at the
        end (the codes are read there)."""
        main = torch.cuda.current_stream()
        for st in self._part_streams:
            st.wait_stream(main)
        for _ in range(k):
            for p, st in zip(self.parts, self._part_streams):
                with torch.cuda.stream(st):
                    p.graph.replay()
        for st in self._part_streams:
            main.wait_stream(st)


def decode_parts(batch_size: int, device, parts: Optional[int] = None) -> int:
    """How many concurrent batch-slice chains a decode engine uses: ``parts`` (else ``DALLE_AMD_DECODE_PARTS``),
    default 2 for batches of 32 and more (1 below); 4 chains measured 17.7 vs 20.1 images/s with per-part graphs
    (profiles/r6_decode_replay_host.txt). Reference model, batch 64, same box
    (profiles/r2_decode_split_parts.txt): 2 parts 3.53 ms per image-position step and 17.0 images/s vs
    3.74 ms / 16.0 for one chain; 4 parts 4.0-6.1 ms. With the decode kernels at a few us each, two
    half-batch chains overlap one chain's latency-bound kernels with the other's (it measured +1 % when
    the skinny GEMMs still carried their split-K hand-off)."""
    if parts is None and os.environ.get("DALLE_AMD_DECODE_PARTS"):
        parts = int(os.environ["DALLE_AMD_DECODE_PARTS"])
    n = max(1, int(parts if parts is not None else (2 if batch_size >= 32 else 1)))
    return n if batch_size % n == 0 else 1


def make_decode_engine(model, batch_size: int, device=None, guided: bool = False, row_params: bool = False):
    """``row_params``: an engine with per-picture sampling parameters (``DecodeEngine``).
    ``guided``: an engine for classifier-free guidance (two rows per picture). The split into parts is decided
    on the row count; the skinny GEMM limit is 64 rows, so at most 32 guided pictures stay on that path."""
    device = device or next(model.parameters()).device
    parts = decode_parts(2 * batch_size if guided else batch_size, device)
    if parts > 1 and batch_size % parts == 0:
        eng = SplitDecodeEngine(model, batch_size, device=device, parts=parts, guided=guided, row_params=row_params)
        if eng.use_hip:
            return eng
    return DecodeEngine(model, batch_size, device=device, guided=guided, row_params=row_params)
