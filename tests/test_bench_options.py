"""bench.py's run modes: a run without --full keeps the headline and switches every other leg off, and
--dump-outputs writes what the last timed step computed (the same file for the same arguments)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_switches_every_other_leg_off(bench, monkeypatch):
    args = _parse(bench, monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not args.full and args.dump_outputs is None and args.cpu_seconds > 0
    bench.headline_only(args)
    assert args.steps == 7 and args.warmup == 2
    assert all(getattr(args, f) for f in ("no_extras", "no_sharded", "no_train", "no_shard_train", "no_cascade",
                                          "no_pipe", "no_probes", "no_uniform_leg"))
    assert args.cpu_seconds == 0 and args.sim_ranks == 0 and not args.cascade_sharded
    full = _parse(bench, monkeypatch, ["--full", "--no-pipe", "--dump-outputs", "d"])
    assert full.full and full.no_pipe and not full.no_extras and full.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(bench, monkeypatch, tmp_path):
    import torch

    x = torch.arange(40 * 6, dtype=torch.float32).reshape(40, 6)
    bench.dump_outputs(str(tmp_path / "whole"), x)
    got = np.load(tmp_path / "whole" / "pooled.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, x.numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 10 * 6 * 4 + 5)  # room for 10 of the 40 rows
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), x)
    a, b = np.load(tmp_path / "a" / "pooled.npy"), np.load(tmp_path / "b" / "pooled.npy")
    assert a.shape == (10, 6) and a.nbytes <= bench.DUMP_BYTES_MAX
    np.testing.assert_array_equal(a, b)
    rows = (a[:, 0] / 6).astype(int)
    assert len(set(rows)) == 10 and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(a, x.numpy()[rows])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_output(cuda, tmp_path):
    """One small plain run end to end: the line keeps its fields, no other leg ran, and pooled.npy holds the
    encoder's output for the batch of the last timed step, bit for bit."""
    import torch

    from recommendflow_amd.backend.encoder.sparse_encoder import FusedSparseEncoder, SlotSpec
    from recommendflow_amd.config_parser.configuration import Configuration
    from recommendflow_amd.runtime.batch import synthetic_batch

    B, rows, dim, steps, batches = 48, 100_000, 16, 3, 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(B), "--batches", str(batches), "--table-rows", str(rows), "--dim", str(dim),
                        "--dump-outputs", str(tmp_path / "out")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["steps"] == steps and j["unit"] == "examples/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] > 0 and j["value"] == pytest.approx(B / j["ms_per_step"] * 1e3, rel=1e-2)
    assert j["probes"] is None and j["cpu_baseline"] is None and j["extras"] is None and j["cfg4_sharded"] is None
    assert j["roofline"]["uniform"] is None
    assert os.listdir(tmp_path / "out") == ["pooled.npy"]
    got = np.load(tmp_path / "out" / "pooled.npy")

    feats = Configuration(os.path.join(ROOT, "tests", "golden", "conf", "base_recall_sdpa.yaml")).features.hashing_features
    specs = [SlotSpec(f.name, rows // (2 * len(feats)), tuple(f.hash_seeds), f.pooling.value) for f in feats]
    enc = FusedSparseEncoder(specs, dim, table_dtype=torch.float32, seed=2023)
    hb = synthetic_batch(B, [bool(f.multivalued) for f in feats], seed=1234 + (steps - 1) % batches)
    want = enc(hb.to("cuda")).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
