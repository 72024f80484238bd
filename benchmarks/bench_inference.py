#!/usr/bin/env python3
"""BASELINE config 5: text->image top-k sampling, batch 64 on one MI355X, hipGraph-replayed decode.

Reference model recipe (64 layers, 5 shared blocks, reversible) with random-init weights and a
random-init VQGAN decoder; prints one JSON line with images/s (end-to-end: prefill + 1024 decode
steps + VQGAN decode) and the per-token decode latency.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dalle_amd.config import get_config  # noqa: E402
from dalle_amd.models.dalle import DALLE  # noqa: E402
from dalle_amd.models.vqgan import VQGanVAE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--model", default="reference")
    ap.add_argument("--top-k", type=int, default=256)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-vae", action="store_true")
    ap.add_argument("--same-caption", action="store_true",
                    help="one caption repeated over the batch, as inference/run_inference.py generates (the decode "
                         "attention then reads the text keys from one cache row); default: a distinct caption per row")
    ap.add_argument("--cond-scale", type=float, default=1.0,
                    help="classifier-free guidance scale: other than 1, a guided engine (two rows per picture; at most 32 "
                         "pictures stay on the skinny GEMM path)")
    ap.add_argument("--no-share-src", action="store_true",
                    help="guided: every row reads the text keys from its own cache (default: null rows from the first "
                         "null row, caption rows from row 0 when the captions are equal)")
    ap.add_argument("--inpaint-rows", default=None, metavar="A:B",
                    help="inpainting: regenerate grid rows A..B-1 of a fixed random picture, keep the rest "
                         "(DALLE.generate_images(img=..., img_mask=...))")
    ap.add_argument("--no-prefill-kept", action="store_true",
                    help="inpainting: the kept codes before the region go through decode steps, not the batched prefill")
    ap.add_argument("--no-skip-tail", action="store_true",
                    help="inpainting: run the decode steps after the region's last position too")
    ap.add_argument("--inpaint-ab", type=int, default=0, metavar="N",
                    help="N rounds over the generation modes, alternating (sampling only, no VAE decode): full; 448 forced "
                         "codes as decode steps; the same as a suffix mask through the batched prefill; --inpaint-rows "
                         "(default 8:24) with both savings, with skip_tail only, with neither. Prints medians and spread")
    ap.add_argument("--row-params", action="store_true",
                    help="per-picture sampling parameters: the call goes through a row-parameter engine "
                         "(DecodeEngine(row_params=True)) with uniform tables (--top-k for every picture)")
    ap.add_argument("--row-mix", action="store_true",
                    help="with --row-params: the first half of the pictures top-k (--top-k), the second half nucleus 0.9")
    ap.add_argument("--row-ab", type=int, default=0, metavar="N",
                    help="N rounds, alternating (sampling only, no VAE decode): the plain engine's scalar call; a row-parameter "
                         "engine with uniform tables; the same with the --row-mix tables. Prints medians and spread")
    ap.add_argument("--profile-steps", type=int, default=0,
                    help="batched caption prefill + N image-position decode steps (graph replays unless --no-graph), "
                         "then exit (rocprof)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = get_config(args.model)
    model = DALLE(cfg).to(dev).eval()
    if not args.no_vae:
        model.vae = VQGanVAE().to(dev).eval()
    text = torch.randint(2, cfg.num_text_tokens, (1 if args.same_caption else args.batch, cfg.text_seq_len), device=dev)
    text = text.expand(args.batch, -1).contiguous()
    use_graph = not args.no_graph
    from dalle_amd.models.generation import make_decode_engine
    guided = args.cond_scale != 1.0
    gen_kw = {"cond_scale": args.cond_scale} if guided else {}
    S, L = cfg.image_fmap_size, cfg.image_seq_len
    picture = torch.randint(0, cfg.num_image_tokens, (args.batch, L), device=dev,
                            generator=torch.Generator(device=dev).manual_seed(1))

    def rows_mask(spec):
        a, b = (int(v) for v in spec.split(":"))
        if not 0 <= a < b <= S:
            raise SystemExit(f"--inpaint-rows {spec}: need 0 <= A < B <= {S}")
        m = torch.zeros(args.batch, S, S, dtype=torch.bool, device=dev)
        m[:, a:b] = True
        return m

    if args.inpaint_rows:
        gen_kw.update(img=picture, img_mask=rows_mask(args.inpaint_rows), prefill_kept=not args.no_prefill_kept,
                      skip_tail=not args.no_skip_tail)
    half = args.batch // 2
    uniform = {"top_k": [args.top_k] * args.batch}
    mixed = {"top_k": [args.top_k] * half + [0] * (args.batch - half), "top_p": [1.0] * half + [0.9] * (args.batch - half)}
    samp = {"top_k": args.top_k}
    if args.row_params:
        samp = mixed if args.row_mix else uniform
    slot = ("_guided_row_decode_engine" if guided else "_row_decode_engine") if args.row_params else (
        "_guided_decode_engine" if guided else "_decode_engine")
    eng = make_decode_engine(model, args.batch, device=dev, **({"guided": True} if guided else {}),
                             **({"row_params": True} if args.row_params else {}))
    setattr(model, slot, eng)
    if guided:
        for e in getattr(eng, "parts", [eng]):
            e.share_src = not args.no_share_src
    parts = getattr(eng, "nparts", 1)
    tb = model.prepare_text(text)
    prefill = getattr(eng, "prefill_parallel", eng.prefill)
    # warm-up generate (captures the step graph)
    t = time.perf_counter()
    model.generate_images(text, **samp, use_graph=use_graph, **gen_kw)
    torch.cuda.synchronize()
    print(f"# warm-up generate done: {time.perf_counter() - t:.2f}s", file=sys.stderr, flush=True)
    t = time.perf_counter()
    prefill(tb)
    torch.cuda.synchronize()
    print(f"# batched prefill of {cfg.text_len} caption positions: {(time.perf_counter() - t) * 1e3:.1f} ms", file=sys.stderr,
          flush=True)
    if args.row_ab:
        base = {"cond_scale": args.cond_scale} if guided else {}
        variants = [("plain engine, scalar call", {"top_k": args.top_k}), ("row engine, uniform tables", uniform),
                    ("row engine, half top-k / half nucleus 0.9", mixed)]
        times = {name: [] for name, _ in variants}
        for rnd in range(args.row_ab + 1):  # round 0 is the warm-up of every variant (engines built, graphs captured)
            for name, kw in variants:
                torch.cuda.synchronize()
                t = time.perf_counter()
                model.generate_images(text, use_graph=use_graph, return_codes=True, **base, **kw)
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(time.perf_counter() - t)
            print(f"# round {rnd} done", file=sys.stderr, flush=True)
        res = {}
        for name, ts in times.items():
            ts = sorted(ts)
            res[name] = {"median_s": round(ts[len(ts) // 2], 4), "min_s": round(ts[0], 4), "max_s": round(ts[-1], 4),
                         "calls": len(ts)}
        print(json.dumps({"metric": "sampling parameters per picture, seconds per call (sampling only, alternating rounds)",
                          "batch": args.batch, "model": args.model, "top_k": args.top_k, "decode_parts": parts,
                          "graph": use_graph, "variants": res}), flush=True)
        return
    if args.inpaint_ab:
        k = int(0.4375 * L)
        band = rows_mask(args.inpaint_rows or f"{S // 4}:{3 * S // 4}")
        base = {"cond_scale": args.cond_scale} if guided else {}
        variants = [
            ("full generation", {}),
            (f"prefix {k} as decode steps", dict(img=picture, num_init_img_tokens=k)),
            (f"suffix mask from {k}, prefill_kept", dict(img=picture, img_mask=torch.arange(L, device=dev).expand(args.batch, L) >= k)),
            ("rows band, prefill_kept + skip_tail", dict(img=picture, img_mask=band)),
            ("rows band, skip_tail only", dict(img=picture, img_mask=band, prefill_kept=False)),
            ("rows band, neither", dict(img=picture, img_mask=band, prefill_kept=False, skip_tail=False)),
        ]
        times = {name: [] for name, _ in variants}
        for rnd in range(args.inpaint_ab + 1):  # round 0 is the warm-up of every variant
            for name, kw in variants:
                torch.cuda.synchronize()
                t = time.perf_counter()
                model.generate_images(text, top_k=args.top_k, use_graph=use_graph, return_codes=True, **base, **kw)
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(time.perf_counter() - t)
            print(f"# round {rnd} done", file=sys.stderr, flush=True)
        res = {}
        for name, ts in times.items():
            ts = sorted(ts)
            res[name] = {"median_s": round(ts[len(ts) // 2], 4), "min_s": round(ts[0], 4), "max_s": round(ts[-1], 4),
                         "calls": len(ts)}
            print(f"# {name:40s} median {res[name]['median_s']:.4f} s  [{ts[0]:.4f}, {ts[-1]:.4f}]  n={len(ts)}", file=sys.stderr)
        print(json.dumps({"metric": "generation modes, seconds per call (sampling only, alternating rounds)", "batch": args.batch,
                          "model": args.model, "top_k": args.top_k, "rows": args.inpaint_rows or f"{S // 4}:{3 * S // 4}",
                          "decode_parts": parts, "graph": use_graph, "variants": res}), flush=True)
        return
    if args.profile_steps:
        # image positions only (the text-key part of every sparse pattern is read from here on)
        if use_graph and hasattr(eng, "replay_steps"):
            eng.replay_steps(args.profile_steps)
        for _ in range(0 if (use_graph and hasattr(eng, "replay_steps")) else args.profile_steps):
            eng.graph.replay() if use_graph else eng._image_step()
        torch.cuda.synchronize()
        return
    # one more untimed generate: the first one after the standalone prefill above runs ~0.3 s slow
    # (profiles/r3_decode_partials_cols.txt), which is not the steady-state rate
    model.generate_images(text, **samp, use_graph=use_graph, **gen_kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.iters):
        out = model.generate_images(text, **samp, use_graph=use_graph, **gen_kw)
        torch.cuda.synchronize()
        print(f"# generate {i}: {time.perf_counter() - t0:.2f}s", file=sys.stderr, flush=True)
    el = (time.perf_counter() - t0) / args.iters
    # sampling alone (no VAE): batched caption prefill + 1024 decode steps, per sampled image token
    t2 = time.perf_counter()
    model.generate_images(text, **samp, use_graph=use_graph, return_codes=True, **gen_kw)
    torch.cuda.synchronize()
    codes_s = time.perf_counter() - t2
    eng = getattr(model, slot)
    # decode-only timing: 256 image positions right after the batched caption prefill (every step
    # reads the 256 text keys of each layer's cache plus its local image keys). 256, not 64: the two
    # chains' per-part graphs run free and the window ends on the later one (~19 ms per window,
    # profiles/r6_decode_replay_host.txt), which a 64-step window would spread as +0.3 ms per step
    NDEC = 256
    prefill(tb)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if use_graph and hasattr(eng, "replay_steps"):
        eng.replay_steps(NDEC)
    for _ in range(0 if (use_graph and hasattr(eng, "replay_steps")) else NDEC):
        eng.graph.replay() if use_graph else eng._step()
    torch.cuda.synchronize()
    per_tok = (time.perf_counter() - t1) / NDEC
    print(json.dumps({"metric": "text->image generation throughput (batch 64, top-k, hipGraph decode)",
                      "value": round(args.batch / el, 3), "unit": "images/s", "n_gpus": 1,
                      "seconds_per_batch": round(el, 3), "ms_per_decode_step": round(per_tok * 1e3, 3),
                      "decode_step_positions": f"image positions {cfg.text_len - 1}..{cfg.text_len + NDEC - 2}",
                      "ms_per_image_token": round(codes_s / cfg.image_seq_len * 1e3, 3),
                      "sampling_seconds": round(codes_s, 3), "decode_parts": parts,
                      "batch": args.batch, "model": args.model, "depth": cfg.depth, "graph": use_graph,
                      "vae": not args.no_vae, "out_shape": list(out.shape), "dtype": "bf16",
                      "captions": "one repeated" if args.same_caption else "distinct per row",
                      "text_shared": [int(e.text_shared.item()) for e in getattr(eng, "parts", [eng])],
                      **({"cond_scale": args.cond_scale, "rows": 2 * args.batch, "share_src": not args.no_share_src} if guided else {}),
                      **({"row_params": "mixed" if args.row_mix else "uniform"} if args.row_params else {}),
                      "data": "random-init weights, synthetic captions"}), flush=True)


if __name__ == "__main__":
    main()
