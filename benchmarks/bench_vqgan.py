#!/usr/bin/env python3
"""K20: VQGAN f8 decoder (the LAION vqgan_gumbel_f8 geometry: 32x32 codes -> 256x256 RGB) on the HIP
kernels vs the PyTorch (MIOpen) decoder, batch 64 by default. One JSON line: ms per batch, images/s,
executed TFLOP/s of the 3x3 convolutions, max |HIP - torch| over the batch.

``--encode``: the encoder instead (K19): ``get_codebook_indices`` of 256x256 pictures on the HIP kernels
(``hip_encoder = True``) vs the PyTorch path (``False``) in one process, the two alternated round by round after a
warm-up of each; per path the median and the spread of the per-call times over all rounds and the peak device memory
of a call. One JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dalle_amd.models.vqgan import VQGanVAE  # noqa: E402


def conv_flops(dec, side):
    """3x3-conv FLOPs of one decoded image (taming Decoder at latent side `side`)."""
    tot, res = 0, side
    mods = [("conv_in", dec.conv_in, res)]
    mods += [(n, m, res) for n, m in dec.mid.named_modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]
    for i_level in reversed(range(dec.num_resolutions)):
        up = dec.up[i_level]
        for blk in up.block:
            mods += [("c", blk.conv1, res), ("c", blk.conv2, res)]
        if i_level != 0:
            res *= 2
            mods.append(("u", up.upsample.conv, res))
    mods.append(("out", dec.conv_out, res))
    for _, m, r in mods:
        tot += 2 * r * r * m.in_channels * m.out_channels * 9
    return tot


def encode(vae, args, dev):
    side = vae.image_size
    images = torch.rand(args.batch, 3, side, side, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def call(hip):
        vae.hip_encoder = hip
        assert vae.use_hip_encoder(side, side) == hip, "the HIP encoder does not support this model"
        return vae.get_codebook_indices(images)

    def timed(hip):
        times = []
        for _ in range(args.iters):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call(hip)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        return times

    res = {}
    for hip in (True, False):  # warm-up of every shape, then the peak memory of one call
        out = call(hip)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = call(hip)
        torch.cuda.synchronize()
        res[hip] = {"codes": out, "peak": torch.cuda.max_memory_allocated() - base, "t": []}
        del out
    for _ in range(args.rounds):
        for hip in (True, False):
            res[hip]["t"] += timed(hip)

    def stats(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    (hm, hlo, hhi), (tm, tlo, thi) = stats(res[True]["t"]), stats(res[False]["t"])
    agree = (res[True]["codes"] == res[False]["codes"]).float().mean().item()
    print(json.dumps({"bench": "vqgan_encode", "batch": args.batch, "side": side, "calls_per_path": len(res[True]["t"]),
                      "hip_ms": round(hm * 1e3, 2), "hip_ms_min_max": [round(hlo * 1e3, 2), round(hhi * 1e3, 2)],
                      "torch_ms": round(tm * 1e3, 2), "torch_ms_min_max": [round(tlo * 1e3, 2), round(thi * 1e3, 2)],
                      "hip_images_per_s": round(args.batch / hm, 1), "torch_images_per_s": round(args.batch / tm, 1),
                      "speedup": round(tm / hm, 2),
                      "hip_peak_mib": round(res[True]["peak"] / 2 ** 20, 1), "torch_peak_mib": round(res[False]["peak"] / 2 ** 20, 1),
                      "codes_agree": round(agree, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--encode", action="store_true", help="time get_codebook_indices (HIP vs PyTorch encoder)")
    ap.add_argument("--rounds", type=int, default=5, help="--encode: alternated HIP / PyTorch rounds of --iters calls")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = VQGanVAE().to(dev).eval()
    if args.encode:
        return encode(vae, args, dev)
    codes = torch.randint(0, vae.num_tokens, (args.batch, 1024), device=dev)

    def run(torch_path):
        vae.hip_decoder = not torch_path  # the A/B switch of VQGanVAE.decode
        assert vae.use_hip_decoder(32, 32) == (not torch_path)
        out = vae.decode(codes)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.iters):
            out = vae.decode(codes)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t) / args.iters

    img, t_hip = run(False)
    ref, t_torch = run(True)
    fl = conv_flops(vae.decoder, 32) * args.batch
    print(json.dumps({"batch": args.batch, "hip_ms": round(t_hip * 1e3, 2), "torch_ms": round(t_torch * 1e3, 2),
                      "hip_images_per_s": round(args.batch / t_hip, 1), "torch_images_per_s": round(args.batch / t_torch, 1),
                      "hip_conv_tflops": round(fl / t_hip / 1e12, 1), "speedup": round(t_torch / t_hip, 2),
                      "max_abs_diff": round((img - ref).abs().max().item(), 4),
                      "mean_abs_diff": round((img - ref).abs().mean().item(), 5)}), flush=True)


if __name__ == "__main__":
    main()
