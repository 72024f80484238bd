#!/usr/bin/env python3
"""Text -> image serving on MI355X: an HTTP front-end over the hipGraph decode engine, on one GPU or on
every GPU of a node (``--devices all``: one model copy, decode-engine cache and worker thread per GPU;
each request goes to the device with the fewest images queued).

The reference only has the offline batch script (``inference/run_inference.py``); this is its online
counterpart for deployment. Requests are queued and a single GPU worker thread forms batches:

* requests with the same sampling parameters (temperature, top-k, top-p, guidance scale) share a batch; the worker
  waits at most ``--batch-window-ms`` for more work after the first request, up to ``--max-batch``
  images (the decode engine's skinny-GEMM path covers batches <= 64);
* the batch is padded to the next power of two and run through a decode engine (two concurrent
  :class:`DecodeEngine` chains from batch 32 on) cached per
  padded size, so every shape's hipGraph is captured once and replayed for every later batch;
* ``cond_scale`` other than 1 (classifier-free guidance) runs on a guided engine, cached per padded picture count
  beside the plain ones; the scale itself is a device scalar, so every scale replays the same graph;
* ``init_image`` (with ``mask``: inpainting, white = regenerate; without: the first ``num_init_img_tokens`` codes are
  kept) edits a picture: requests with and without pictures share a batch under the same sampling parameters -- a row
  without a picture regenerates every position, which is the ordinary path, bit for bit;
* ``seed`` (an int64) makes a request replayable: image ``i`` of the request samples with the noise key
  ``(seed, noise_row = i)`` on a row-parameter engine (``DecodeEngine(row_params=True)``), whatever its batch slot and
  neighbours, and the response echoes the seed. Codes are bitwise reproducible at the same padded batch size and engine
  kind (the decode GEMMs round per batch shape). Without ``--mix-params`` a seeded request batches only with seeded
  requests of the same parameters, and a request without a seed takes the plain path (its response's seed is null:
  that path's noise is keyed by the batch slot and cannot be replayed per picture);
* ``--mix-params`` (``mix_params=True``; off by default): the batching key shrinks to "guided or not". Every batch
  runs on a row-parameter engine with one temperature / top-k / top-p / guidance scale / seed per picture, so requests
  with different settings share a batch, and a request without a seed gets one drawn at ``submit``;
* codes are decoded by the VQGAN and returned as base64 PNGs together with per-request timings.

Endpoints: ``POST /generate`` ``{"prompts": [...], "images_per_prompt": 1, "temperature": 1.0,
"top_k": 256, "top_p": 1.0, "cond_scale": 1.0, "init_image": <base64 PNG>, "mask": <base64 PNG>,
"num_init_img_tokens": null, "seed": null}``, ``GET /health``, ``GET /stats``. ``create_app`` builds the app around
an already-loaded model (tests, embedding into another service); ``main`` loads weights like
``run_inference.py`` and starts uvicorn.
"""
from __future__ import annotations

import argparse
import base64
import copy
import io
import os
import queue
import secrets
import sys
import threading
import time
from concurrent.futures import Future
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dalle_amd.models.generation import DecodeEngine, make_decode_engine  # noqa: E402
from dalle_amd.utils.logging import get_logger  # noqa: E402

logger = get_logger(__name__)


def _png_b64(img: np.ndarray) -> str:
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray((np.clip(img, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)).save(buf, format="PNG")
    return base64.b64encode(buf.getvalue()).decode("ascii")


def _b64_image(data: str, mode: str):
    from PIL import Image

    return Image.open(io.BytesIO(base64.b64decode(data))).convert(mode)


class _Job:
    def __init__(self, prompts: List[str], n: int, key: tuple, image=None, regen=None, params=None, seed=None):
        self.prompts, self.n, self.key = prompts, n, key
        # params (temperature, top_k, top_p, cond_scale) and the seed of a job that runs on a row-parameter engine
        # (``rows``); a plain job's parameters are its key
        self.params, self.seed, self.rows = params, seed, params is not None
        self.image, self.regen = image, regen  # (L,) codes and (L,) bool (True = regenerate), or None: no picture
        self.future: Future = Future()
        self.t_submit = time.perf_counter()

    @property
    def images(self) -> int:
        return len(self.prompts) * self.n


class BatchingGenerator:
    """Owns the model on one device; ``submit`` is thread-safe, all GPU work happens in one thread."""

    def __init__(self, model, tokenizer, device, max_batch: int = 64, batch_window_ms: float = 20.0,
                 mix_params: bool = False):
        self.model, self.tokenizer, self.device = model, tokenizer, torch.device(device)
        self.mix_params = bool(mix_params)
        self.max_batch = max(1, int(max_batch))
        self.window = batch_window_ms / 1000.0
        self.q: "queue.Queue[Optional[_Job]]" = queue.Queue()
        self.engines: Dict[int, DecodeEngine] = {}
        self.guided_engines: Dict[int, DecodeEngine] = {}  # classifier-free guidance, by padded picture count
        self.row_engines: Dict[int, DecodeEngine] = {}  # per-picture sampling parameters (seeded or mixed batches)
        self.guided_row_engines: Dict[int, DecodeEngine] = {}
        self.stats = {"requests": 0, "images": 0, "batches": 0, "gpu_seconds": 0.0}
        self._held: List[_Job] = []  # popped while batching but with other sampling parameters
        self._vae_lock = threading.Lock()  # pictures are encoded in the submitting thread
        self._thread = threading.Thread(target=self._loop, name="dalle-serve-worker", daemon=True)
        self._thread.start()

    # -- API ------------------------------------------------------------------------------------
    def submit(self, prompts: List[str], images_per_prompt: int = 1, temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, cond_scale: float = 1.0, init_image=None, mask=None, num_init_img_tokens=None,
               seed: Optional[int] = None) -> Future:
        """``seed``: image ``i`` of the request draws its noise from ``(seed, noise_row = i)``; the result carries it.
        ``init_image``: a base64 PNG (encoded by the model's VQGAN) or the picture's codes (a sequence of
        image_seq_len integers; works without a VAE). ``mask``: a base64 PNG (white = regenerate, framed like the
        picture) or an array over the codes / pixels (``dalle_amd.models.dalle.code_mask``). Without a mask the first
        ``num_init_img_tokens`` codes (default 0.4375 of them) are kept. The picture applies to every image of the
        request."""
        if cond_scale < 0:
            raise ValueError("cond_scale must be >= 0")
        image, regen = self._picture(init_image, mask, num_init_img_tokens)
        params = (float(temperature), int(top_k), float(top_p), float(cond_scale))
        if seed is not None and not -(2 ** 63) <= int(seed) < 2 ** 63:
            raise ValueError("seed must fit 64 bits")
        if self.mix_params:  # one key per engine kind; a seed of the request's own if it brought none
            job = _Job(list(prompts), int(images_per_prompt), ("mix", params[3] != 1.0), image, regen, params,
                       secrets.randbits(62) if seed is None else int(seed))
        elif seed is not None:  # seeded requests of the same parameters share a batch, apart from the unseeded ones
            job = _Job(list(prompts), int(images_per_prompt), params + ("seeded",), image, regen, params, int(seed))
        else:
            job = _Job(list(prompts), int(images_per_prompt), params, image, regen)
        if not job.prompts or job.n < 1:
            raise ValueError("need at least one prompt and images_per_prompt >= 1")
        if job.images > self.max_batch:
            raise ValueError(f"a request may ask for at most {self.max_batch} images")
        self.q.put(job)
        return job.future

    def close(self):
        self.q.put(None)
        self._thread.join(timeout=60)

    def _picture(self, init_image, mask, num_init_img_tokens):
        """A request's picture arguments -> ((L,) codes, (L,) bool regenerate mask) on the host, or (None, None)."""
        from dalle_amd.models.dalle import code_mask

        L, g, vae = self.model.image_seq_len, self.model.cfg.image_fmap_size, self.model.vae
        if init_image is None:
            if mask is not None or num_init_img_tokens is not None:
                raise ValueError("mask and num_init_img_tokens need init_image")
            return None, None
        if mask is not None and num_init_img_tokens is not None:
            raise ValueError("give either mask (inpainting) or num_init_img_tokens (a kept prefix), not both")
        size = None if vae is None else getattr(vae, "image_size", None)
        if isinstance(init_image, str):
            if vae is None:
                raise ValueError("a picture file needs a VAE to encode it; pass the picture's codes instead")
            from run_inference import load_init_image

            pic = load_init_image(io.BytesIO(base64.b64decode(init_image)), size)
            with self._vae_lock:
                image = vae.get_codebook_indices(pic.unsqueeze(0).to(self.device))[0].long().cpu()
        else:
            image = torch.as_tensor(init_image).reshape(-1)
            if image.dtype.is_floating_point or image.dtype == torch.bool:
                raise ValueError("init_image codes must be integers")
            image = image.long().cpu()
        if image.numel() != L:
            raise ValueError(f"init_image must give {L} image codes, got {image.numel()}")
        if mask is None:
            k = int(0.4375 * L) if num_init_img_tokens is None else int(num_init_img_tokens)
            if not 0 <= k < L:
                raise ValueError(f"num_init_img_tokens must be in [0, {L}), got {k}")
            return image, torch.arange(L) >= k
        if isinstance(mask, str):
            if size is None:
                raise ValueError("a mask file is over the pixels and needs a VAE; pass a mask over the codes instead")
            from run_inference import load_mask

            mask = load_mask(io.BytesIO(base64.b64decode(mask)), size)
        return image, code_mask(torch.as_tensor(mask).unsqueeze(0), 1, g, size)[0].cpu()

    # -- worker ---------------------------------------------------------------------------------
    def _next(self, timeout: Optional[float], held: bool = True) -> Optional[_Job]:
        if held and self._held:
            return self._held.pop(0)
        try:
            return self.q.get(timeout=timeout) if timeout is None or timeout > 0 else self.q.get_nowait()
        except queue.Empty:
            return None

    def _loop(self):
        torch.set_grad_enabled(False)
        if self.device.type == "cuda":
            # this thread's current device = the generator's: streams, hipGraph captures and the native
            # ops' stream lookups must bind to that GPU, not to GPU 0
            torch.cuda.set_device(self.device)
            # and a (non-blocking) stream of the worker's own: work on the legacy default stream would have to
            # synchronise with every blocking stream -- including a hipGraph capture running in another
            # generator's thread on the same GPU, which then fails ("legacy stream depend on a capturing stream")
            with torch.cuda.stream(torch.cuda.Stream(device=self.device)):
                self._serve()
        else:
            self._serve()

    def _serve(self):
        while True:
            first = self._next(None)
            if first is None:
                return
            batch, size = [first], first.images
            deadline = time.perf_counter() + self.window
            # same-parameter jobs set aside earlier join first, then new arrivals until the window closes
            later = [j for j in self._held if j.key != first.key]
            for j in [j for j in self._held if j.key == first.key]:
                if size + j.images <= self.max_batch:
                    batch.append(j)
                    size += j.images
                else:
                    later.append(j)
            self._held = later
            while size < self.max_batch:
                job = self._next(deadline - time.perf_counter(), held=False)
                if job is None:
                    break
                if job.key == first.key and size + job.images <= self.max_batch:
                    batch.append(job)
                    size += job.images
                else:
                    self._held.append(job)
                    if job.key == first.key:  # no room: it opens the next batch
                        break
            try:
                self._run(batch)
            except Exception as e:  # noqa: BLE001 - report to the callers, keep serving
                logger.exception("generation failed")
                for job in batch:
                    if not job.future.done():
                        job.future.set_exception(e)

    def _ids(self, prompts: List[str]) -> torch.Tensor:
        L = self.model.text_seq_len
        out = torch.full((len(prompts), L), 1, dtype=torch.long)  # pad = eos = 1 (task.py:59)
        for i, p in enumerate(prompts):
            ids = self.tokenizer(p, add_special_tokens=False, max_length=L, truncation=True)["input_ids"][:L]
            if ids:
                out[i, : len(ids)] = torch.tensor(ids, dtype=torch.long)
        return out

    def _run(self, batch: List[_Job]):
        prompts = [p for job in batch for p in job.prompts for _ in range(job.n)]
        n = len(prompts)
        padded = 1
        while padded < n:
            padded *= 2
        padded = min(padded, self.max_batch) if n <= self.max_batch else n
        ids = self._ids(prompts + [prompts[-1]] * (padded - n)).to(self.device)
        rows = batch[0].rows
        if rows:
            # one table row per picture: the job's parameters and seed, image i of the job on noise row i; the padded
            # rows copy the last row, as they do for pictures and masks
            per = [job.params + (job.seed, i) for job in batch for i in range(job.images)]
            per += [per[-1]] * (padded - n)
            temperature, top_k, top_p, cond_scale, seeds, noise = (list(c) for c in zip(*per))
            guided = any(job.params[3] != 1.0 for job in batch)
            cache = self.guided_row_engines if guided else self.row_engines
        else:
            temperature, top_k, top_p, cond_scale = batch[0].key
            guided = cond_scale != 1.0
            cache = self.guided_engines if guided else self.engines
        eng = cache.get(padded)
        if eng is None:
            eng = cache[padded] = make_decode_engine(self.model, padded, device=self.device, **({"guided": True} if guided else {}),
                                                     **({"row_params": True} if rows else {}))
        kw = {"cond_scale": cond_scale} if guided else {}
        if rows:
            kw.update(seed=seeds, noise_row=noise)
        if any(job.image is not None for job in batch):
            # one mask per row: a row without a picture regenerates everything (the ordinary path); the padded rows
            # copy the last row's picture and mask
            L = self.model.image_seq_len
            image, regen = torch.zeros(padded, L, dtype=torch.long), torch.ones(padded, L, dtype=torch.bool)
            off = 0
            for job in batch:
                if job.image is not None:
                    image[off:off + job.images], regen[off:off + job.images] = job.image, job.regen
                off += job.images
            image[n:], regen[n:] = image[n - 1], regen[n - 1]
            kw.update(image=image.to(self.device), regen=regen.to(self.device))
        t0 = time.perf_counter()
        codes = eng.generate(self.model.prepare_text(ids), temperature=temperature, top_k=top_k, top_p=top_p, **kw)[:n]
        imgs = self.model.vae.decode(codes) if self.model.vae is not None else None
        if self.device.type == "cuda":
            # this worker's stream only (the engines join their part streams into it): a device-wide synchronize is
            # refused while another generator's thread captures a graph on the same GPU, and invalidates that capture
            torch.cuda.current_stream(self.device).synchronize()
        gpu_s = time.perf_counter() - t0
        arr = imgs.permute(0, 2, 3, 1).float().cpu().numpy() if imgs is not None else None
        self.stats["batches"] += 1
        self.stats["gpu_seconds"] += gpu_s
        off = 0
        for job in batch:
            k = job.images
            res = {"images": [_png_b64(a) for a in arr[off:off + k]] if arr is not None else [],
                   "codes": codes[off:off + k].cpu().tolist() if arr is None else None,
                   "batch_images": n, "batch_padded": padded, "generate_seconds": round(gpu_s, 4),
                   "queue_seconds": round(t0 - job.t_submit, 4), "seed": job.seed}
            off += k
            self.stats["requests"] += 1
            self.stats["images"] += k
            job.future.set_result(res)


class MultiDeviceGenerator:
    """One :class:`BatchingGenerator` per device (its own model copy, decode-engine cache and worker
    thread); ``submit`` routes each request to the device with the fewest images in flight, so a node's
    GPUs batch and decode independently. Same interface as a single generator."""

    def __init__(self, model, tokenizer, devices: List[str], max_batch: int = 64, batch_window_ms: float = 20.0,
                 mix_params: bool = False):
        if not devices:
            raise ValueError("need at least one device")
        self.gens: List[BatchingGenerator] = []
        for i, d in enumerate(devices):
            m = model if i == len(devices) - 1 else copy.deepcopy(model)  # the last device takes the original
            self.gens.append(BatchingGenerator(m.to(d).eval(), tokenizer, d, max_batch, batch_window_ms, mix_params))
        self.max_batch = self.gens[0].max_batch
        self._inflight = [0] * len(self.gens)
        self._lock = threading.Lock()

    @property
    def device(self) -> str:
        return ",".join(str(g.device) for g in self.gens)

    @property
    def engines(self) -> Dict[int, DecodeEngine]:
        out: Dict[int, DecodeEngine] = {}
        for g in self.gens:
            out.update(g.engines)
        return out

    @property
    def row_engines(self) -> Dict[int, DecodeEngine]:
        out: Dict[int, DecodeEngine] = {}
        for g in self.gens:
            out.update(g.row_engines)
        return out

    @property
    def guided_row_engines(self) -> Dict[int, DecodeEngine]:
        out: Dict[int, DecodeEngine] = {}
        for g in self.gens:
            out.update(g.guided_row_engines)
        return out

    @property
    def stats(self) -> Dict[str, float]:
        tot = {"requests": 0, "images": 0, "batches": 0, "gpu_seconds": 0.0}
        for g in self.gens:
            for k in tot:
                tot[k] += g.stats[k]
        tot["per_device_images"] = [g.stats["images"] for g in self.gens]
        return tot

    def submit(self, prompts: List[str], images_per_prompt: int = 1, temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, cond_scale: float = 1.0, init_image=None, mask=None, num_init_img_tokens=None,
               seed: Optional[int] = None) -> Future:
        n = len(prompts) * int(images_per_prompt)
        with self._lock:
            i = min(range(len(self.gens)), key=lambda k: (self._inflight[k], k))
            self._inflight[i] += n
        try:
            fut = self.gens[i].submit(prompts, images_per_prompt, temperature, top_k, top_p, cond_scale, init_image, mask,
                                      num_init_img_tokens, seed)
        except Exception:
            with self._lock:
                self._inflight[i] -= n
            raise

        def done(_f, i=i, n=n):
            with self._lock:
                self._inflight[i] -= n

        fut.add_done_callback(done)
        return fut

    def close(self):
        for g in self.gens:
            g.close()


def parse_devices(spec: str) -> List[str]:
    """``all`` -> every visible GPU; ``0,2`` -> those GPUs; ``cpu`` -> CPU (tests); default: one device."""
    if spec in (None, "", "auto"):
        return ["cuda:0" if torch.cuda.is_available() else "cpu"]
    if spec == "all":
        n = torch.cuda.device_count()
        return [f"cuda:{i}" for i in range(n)] if n else ["cpu"]
    return [d if (d.startswith("cuda") or d == "cpu") else f"cuda:{int(d)}" for d in spec.split(",")]


try:  # the HTTP layer is optional: BatchingGenerator works without fastapi / pydantic
    from pydantic import BaseModel, Field

    class GenerateRequest(BaseModel):
        prompts: List[str]
        images_per_prompt: int = Field(1, ge=1)
        temperature: float = Field(1.0, ge=0.0)
        top_k: int = Field(0, ge=0)
        top_p: float = Field(1.0, gt=0.0, le=1.0)
        cond_scale: float = Field(1.0, ge=0.0)
        init_image: Optional[str] = None  # base64 PNG: the picture to edit
        mask: Optional[str] = None  # base64 PNG, white = regenerate (needs init_image)
        num_init_img_tokens: Optional[int] = Field(None, ge=0)  # without a mask: how many leading codes to keep
        seed: Optional[int] = Field(None, ge=-(2 ** 63), lt=2 ** 63)  # image i draws from (seed, noise row i); echoed back
except ImportError:  # pragma: no cover
    GenerateRequest = None


def create_app(gen):
    """HTTP app around a :class:`BatchingGenerator` or :class:`MultiDeviceGenerator`."""
    from fastapi import FastAPI, HTTPException

    app = FastAPI(title="dalle-mi355x")

    @app.get("/health")
    def health():
        return {"ok": True, "device": str(gen.device), "max_batch": gen.max_batch}

    @app.get("/stats")
    def stats():
        s = dict(gen.stats)
        s["images_per_gpu_second"] = round(s["images"] / s["gpu_seconds"], 3) if s["gpu_seconds"] else None
        s["cached_batch_shapes"] = sorted(gen.engines)
        return s

    @app.post("/generate")
    def generate(req: GenerateRequest):
        try:
            fut = gen.submit(req.prompts, req.images_per_prompt, req.temperature, req.top_k, req.top_p, req.cond_scale,
                             req.init_image, req.mask, req.num_init_img_tokens, req.seed)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        return fut.result()

    return app


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=None, help="DALL-E checkpoint (*.pt); random-init without")
    ap.add_argument("--model-preset", default="reference")
    ap.add_argument("--vqgan", default=None)
    ap.add_argument("--vqgan-config", default=None)
    ap.add_argument("--tokenizer", default="t5-small")
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--devices", default="auto", help='"all" GPUs of the node, a list like "0,1,2,3", or "auto" (one)')
    ap.add_argument("--batch-window-ms", type=float, default=20.0)
    ap.add_argument("--mix-params", action="store_true",
                    help="batch requests with different sampling parameters together, on row-parameter engines")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8000)
    args = ap.parse_args(argv)
    from run_inference import make_model, normalize_state_dict_keys
    from dalle_amd.models.vqgan import VQGanVAE

    torch.set_grad_enabled(False)
    devices = parse_devices(args.devices)
    tokenizer, wrapper = make_model(args.model_preset, args.tokenizer)
    if args.model:
        wrapper.load_state_dict(normalize_state_dict_keys(torch.load(args.model, map_location="cpu", weights_only=True)),
                                strict=False)
    wrapper.model.vae = VQGanVAE(args.vqgan, args.vqgan_config).eval()
    if len(devices) == 1:
        gen = BatchingGenerator(wrapper.model.to(devices[0]).eval(), tokenizer, devices[0], args.max_batch,
                                args.batch_window_ms, args.mix_params)
    else:
        gen = MultiDeviceGenerator(wrapper.model.eval(), tokenizer, devices, args.max_batch, args.batch_window_ms,
                                   args.mix_params)
    logger.info(f"serving on {gen.device}")
    import uvicorn

    uvicorn.run(create_app(gen), host=args.host, port=args.port)


if __name__ == "__main__":
    main()
