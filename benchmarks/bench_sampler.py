#!/usr/bin/env python3
"""The fused decode sampler (csrc/kernels/sample.hip) alone: us per call at the decode shape (32 or 64 rows x 8192
image logits), for top-k 256 / no filter / greedy, to see where its time goes -- and the guided shape (classifier-free
guidance: 64 logit rows, 32 pictures, one workgroup per picture loading both rows) beside the unguided 32- and 64-row
calls. The shapes alternate inside every round (after a warm-up of each); the result is the median over the rounds
with the min-max spread."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dalle_amd.ops.hip_ops import C  # noqa: E402

ROUNDS, CALLS = 7, 200


def main():
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    seed = torch.tensor(7, dtype=torch.int64, device=dev)
    pos = torch.tensor(300, dtype=torch.int32, device=dev)
    scale = torch.tensor([3.0], dtype=torch.float32, device=dev)
    logits = {B: torch.randn(B, 8192, device=dev) * 3 for B in (32, 64)}
    shapes = {"B32": (logits[32], {}), "B64": (logits[64], {}), "G32of64": (logits[64], {"cond_scale": scale})}
    configs = {"topk256": (256, 1.0, 1.0), "nofilter": (0, 1.0, 1.0), "greedy": (0, 1.0, 0.0),
               "topk256_greedy": (256, 1.0, 0.0), "topk256_topp0.9": (256, 0.9, 1.0)}
    times = {f"{s}_{n}": [] for s in shapes for n in configs}
    for rnd in range(ROUNDS + 1):  # round 0: warm-up of every shape, not recorded
        for name, (k, p, t) in configs.items():
            for sname, (lg, kw) in shapes.items():
                for _ in range(10):
                    C().sample_step(lg, k, p, t, seed, pos, **kw)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(CALLS):
                    C().sample_step(lg, k, p, t, seed, pos, **kw)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[f"{sname}_{name}"].append(e0.elapsed_time(e1) / CALLS * 1e3)
    res = {k: round(statistics.median(v), 2) for k, v in times.items()}
    spread = {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
    print(json.dumps({"sampler_us_per_call": res, "min_max": spread, "rounds": ROUNDS, "calls_per_round": CALLS}), flush=True)


if __name__ == "__main__":
    main()
