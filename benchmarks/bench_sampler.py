#!/usr/bin/env python3
"""The fused decode sampler (csrc/kernels/sample.hip) alone: us per call at the decode shape (32 or 64 rows x 8192
image logits), for top-k 256 / no filter / greedy, to see where its time goes -- and the guided shape (classifier-free
guidance: 64 logit rows, 32 pictures, one workgroup per picture loading both rows) beside the unguided 32- and 64-row
calls. Row mode (per-picture parameter tables, the ``ROWS`` instantiations): the same shapes with uniform tables
(``R32`` / ``R64`` / ``RG32of64``, under every config), and a half top-k 256 / half nucleus 0.9 mix at 32 and 64 rows
(``R32_mix`` / ``R64_mix``; a mixed batch takes its slowest row's path). The shapes alternate inside every round (after a warm-up of each); the result is the median over the rounds
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

    def tables(n, k, p, t):
        return {"row_top_k": torch.tensor(k, dtype=torch.int32, device=dev), "row_top_p": torch.tensor(p, dtype=torch.float32, device=dev),
                "row_temperature": torch.tensor(t, dtype=torch.float32, device=dev),
                "row_seed": torch.full((n,), 7, dtype=torch.int64, device=dev), "noise_row": torch.arange(n, dtype=torch.int32, device=dev)}

    row_shapes = {"R32": (logits[32], 32, {}), "R64": (logits[64], 64, {}),
                  "RG32of64": (logits[64], 32, {"cond_scale": scale, "row_cond_scale": torch.full((32,), 3.0, device=dev)})}
    # (logits, keyword arguments) per timed entry; the scalar arguments of a row-mode call are not read
    runs = {f"{s}_{n}": (lg, cfg, kw) for n, cfg in configs.items() for s, (lg, kw) in shapes.items()}
    for n, (k, p, t) in configs.items():
        for s, (lg, rows, kw) in row_shapes.items():
            runs[f"{s}_{n}"] = (lg, (0, 1.0, 1.0), {**kw, **tables(rows, [k] * rows, [p] * rows, [t] * rows)})
    for rows in (32, 64):
        h = rows // 2
        runs[f"R{rows}_mix_topk256_topp0.9"] = (logits[rows], (0, 1.0, 1.0),
                                                tables(rows, [256] * h + [0] * h, [1.0] * h + [0.9] * h, [1.0] * rows))
    times = {name: [] for name in runs}
    for rnd in range(ROUNDS + 1):  # round 0: warm-up of every shape, not recorded
        for name, (lg, (k, p, t), kw) in runs.items():
            for _ in range(10):
                C().sample_step(lg, k, p, t, seed, pos, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                C().sample_step(lg, k, p, t, seed, pos, **kw)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / CALLS * 1e3)
    res = {k: round(statistics.median(v), 2) for k, v in times.items()}
    spread = {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
    print(json.dumps({"sampler_us_per_call": res, "min_max": spread, "rounds": ROUNDS, "calls_per_round": CALLS}), flush=True)


if __name__ == "__main__":
    main()
