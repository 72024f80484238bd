"""Serving with per-picture sampling parameters (inference/serve.py) on the CPU with the tiny model, no VAE (codes are
returned): ``mix_params`` batches requests of different settings together, a seed replays a request's pictures
whatever they were batched with, and without either nothing leaves the plain path."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "inference"))

from dalle_amd.config import DALLEConfig, tiny  # noqa: E402
from dalle_amd.data.tokenizer import HashingTokenizer  # noqa: E402
from dalle_amd.models.dalle import DALLE  # noqa: E402


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    c = tiny(False)
    cfg = DALLEConfig(**{**c.to_dict(), "text_seq_len": 16, "image_size": 64})  # 8x8 codes: fast on CPU
    return DALLE(cfg).eval()


def _gen(model, **kw):
    from serve import BatchingGenerator

    # two pictures fill a batch, so a batch that can be shared runs as soon as its second request arrives and no test
    # waits for the window
    return BatchingGenerator(model, HashingTokenizer(vocab_size=model.cfg.num_text_tokens), "cpu", max_batch=2, **kw)


def test_mixed_parameters_share_a_batch(model):
    gen = _gen(model, batch_window_ms=60000, mix_params=True)
    try:
        a = gen.submit(["a red apple"], temperature=1.0, top_k=32)
        b = gen.submit(["a cat"], temperature=0.0, top_p=0.9)
        ra, rb = a.result(timeout=300), b.result(timeout=300)
        assert ra["batch_images"] == rb["batch_images"] == 2
        assert sorted(gen.row_engines) == [2] and not gen.engines and not gen.guided_row_engines
        greedy = gen.row_engines[2]
        assert greedy.row_params and greedy.row_temperature.tolist() == [1.0, 0.0] and greedy.row_top_k.tolist() == [32, 0]
        assert greedy.noise_row.tolist() == [0, 0] and greedy.row_seed.tolist() == [ra["seed"], rb["seed"]]
    finally:
        gen.close()
    gen = _gen(model, batch_window_ms=50)  # the default: one batch per parameter set
    try:
        a = gen.submit(["a red apple"], temperature=1.0, top_k=32)
        b = gen.submit(["a cat"], temperature=0.0, top_p=0.9)
        ra, rb = a.result(timeout=300), b.result(timeout=300)
        assert ra["batch_images"] == rb["batch_images"] == 1
        assert gen.stats["batches"] == 2 and not gen.row_engines
    finally:
        gen.close()


def test_seed_replay(model):
    gen = _gen(model, batch_window_ms=60000, mix_params=True)
    try:
        a1 = gen.submit(["a red apple"], temperature=1.0, top_k=32, seed=7)
        b = gen.submit(["a cat"], temperature=1.0, top_k=32)
        ra1, rb = a1.result(timeout=300), b.result(timeout=300)
        a2 = gen.submit(["a red apple"], temperature=1.0, top_k=32, seed=7)
        c = gen.submit(["a dog"], temperature=0.7, top_p=0.8)
        ra2, rc = a2.result(timeout=300), c.result(timeout=300)
        assert ra1["batch_images"] == ra2["batch_images"] == 2 and ra1["batch_padded"] == ra2["batch_padded"] == 2
        assert ra1["codes"] == ra2["codes"] and ra1["seed"] == ra2["seed"] == 7
        assert rb["codes"] != rc["codes"]
        # a request without a seed reports the one it drew, and that replays it
        d = gen.submit(["the northern lights"], images_per_prompt=2, top_k=64).result(timeout=300)
        assert isinstance(d["seed"], int) and d["codes"][0] != d["codes"][1]  # one seed, noise rows 0 and 1
        e = gen.submit(["the northern lights"], images_per_prompt=2, top_k=64, seed=d["seed"]).result(timeout=300)
        assert e["codes"] == d["codes"] and e["batch_padded"] == d["batch_padded"] == 2
        with pytest.raises(ValueError, match="64 bits"):
            gen.submit(["x"], seed=2 ** 63)
    finally:
        gen.close()


def test_default_keeps_unseeded_requests_on_the_plain_path(model):
    gen = _gen(model, batch_window_ms=50)
    try:
        r = gen.submit(["a red apple"], images_per_prompt=2, top_k=32).result(timeout=300)
        assert not gen.row_engines and not gen.guided_row_engines and sorted(gen.engines) == [2]
        assert r["seed"] is None and not gen.engines[2].row_params
        # seeded requests of one parameter set share a batch on a row engine, apart from the unseeded ones
        a = gen.submit(["a red apple"], top_k=32, seed=7)
        b = gen.submit(["a cat"], top_k=32, seed=8)
        ra, rb = a.result(timeout=300), b.result(timeout=300)
        assert ra["batch_images"] == rb["batch_images"] == 2 and ra["seed"] == 7 and rb["seed"] == 8
        assert sorted(gen.row_engines) == [2] and sorted(gen.engines) == [2]
        again = gen.submit(["a red apple"], top_k=32, seed=7)
        other = gen.submit(["a bird"], top_k=32, seed=9)
        assert again.result(timeout=300)["codes"] == ra["codes"] and other.result(timeout=300)["batch_images"] == 2
    finally:
        gen.close()


def test_multi_device_generator_passes_the_flag_and_the_seed(model):
    from serve import MultiDeviceGenerator

    gen = MultiDeviceGenerator(model, HashingTokenizer(vocab_size=model.cfg.num_text_tokens), ["cpu"], max_batch=2,
                               batch_window_ms=60000, mix_params=True)
    try:
        a = gen.submit(["a red apple"], top_k=32, seed=7)
        b = gen.submit(["a cat"], temperature=0.5, seed=8)
        assert a.result(timeout=300)["batch_images"] == 2 and b.result(timeout=300)["seed"] == 8
        assert sorted(gen.row_engines) == [2] and not gen.guided_row_engines and not gen.engines
    finally:
        gen.close()
