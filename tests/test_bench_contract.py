"""bench.py contract tests: single-process JSON output and the
2-process gloo (world_size 2) distributed path — the multi-process CPU
coverage for the path torchrun exercises on GPU nodes.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


def run_bench(args, env=None):
    e = dict(os.environ)
    if env:
        e.update(env)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py")] + args,
        capture_output=True, text=True, timeout=420, env=e, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    last = out.stdout.strip().splitlines()[-1]
    return json.loads(last)


class TestPinToReference:
    """A calibration within tolerance of the committed reference profile
    is replaced by it (reproducible runs); any other keeps its own."""

    REF = {"batch_sizes": [1, 64], "itl_ms": [5.0, 10.0],
           "prefill_tokens_per_s": 1000.0, "tolerance": 0.10}

    def pin(self, batches, itl, prefill):
        import bench

        return bench.pin_to_reference(batches, itl, prefill, ref=self.REF)

    def test_within_tolerance_takes_reference(self):
        itl, prefill, dev, pinned = self.pin([1, 64], [5.2, 9.1], 1050.0)
        assert pinned and itl == [5.0, 10.0] and prefill == 1000.0
        assert dev == pytest.approx(0.09)

    def test_jitter_does_not_change_the_result(self):
        a = self.pin([1, 64], [5.03, 9.95], 1004.0)
        b = self.pin([1, 64], [4.97, 10.06], 998.0)
        assert a[:2] == b[:2] and a[3] and b[3]

    @pytest.mark.parametrize("itl,prefill", [
        ([5.6, 10.0], 1000.0),   # one ITL point 12 % slow
        ([5.0, 8.9], 1000.0),    # one ITL point 11 % fast
        ([5.0, 10.0], 1200.0),   # prefill 20 % fast
    ])
    def test_outside_tolerance_keeps_measurement(self, itl, prefill):
        got_itl, got_prefill, dev, pinned = self.pin([1, 64], itl, prefill)
        assert not pinned and got_itl == itl and got_prefill == prefill
        assert dev > 0.10

    def test_other_batch_grid_keeps_measurement(self):
        itl, prefill, dev, pinned = self.pin([1, 32], [5.0, 10.0], 1000.0)
        assert not pinned and itl == [5.0, 10.0] and dev is None

    def test_committed_reference_is_well_formed(self):
        import bench

        with open(bench.REFERENCE_PROFILE) as f:
            ref = json.load(f)
        assert ref["batch_sizes"] == [1, 8, 32, 64, 128, 256]
        assert len(ref["itl_ms"]) == 6
        assert ref["itl_ms"] == sorted(ref["itl_ms"])  # ITL grows with batch
        assert ref["prefill_tokens_per_s"] > 0
        assert 0 < ref["tolerance"] <= 0.10


class TestBenchContract:
    def test_single_process_json(self):
        d = run_bench(["--steps", "6", "--warmup", "2"])
        assert REQUIRED_KEYS <= set(d)
        assert d["unit"] == "%"
        assert d["higher_is_better"] is True
        assert d["scaling"] == "weak"
        assert d["dtype"] == "bf16"
        assert d["data"] == "synthetic"
        assert d["steps"] == 6 and d["warmup"] == 2
        assert 0 <= d["value"] <= 100
        assert d["ms_per_step"] > 0
        assert d["config"]["model"] == "meta-llama/Llama-3.1-8B"

    def test_dump_outputs_repeatable(self, tmp_path):
        """--dump-outputs writes the timed region's replica series and
        scores as float .npy, repeatable across two runs with the same
        arguments (--full must not change them).

        Every input is seeded, and a GPU calibration within tolerance of
        the committed reference profile is settled onto it, so the
        replica series and scores are identical. Only a GPU outside that
        tolerance simulates its own wall-clock measurement; then just
        the shapes repeat. The seeded decode probe must agree to bf16
        rounding: within two ulps of its largest logit."""
        import numpy as np

        dumps, sources, on_gpu = [], set(), False
        for name, extra in (("a", []), ("b", ["--full"])):
            out_dir = tmp_path / name
            d = run_bench(["--steps", "4", "--warmup", "1",
                           "--dump-outputs", str(out_dir)] + extra,
                          env={"WVA_BENCH_GPU_BUSY_S": "0.5"})
            assert d["steps"] == 4
            on_gpu = d["config"]["device"] is not None
            sources.add(d["config"]["service_profile"])
            marker_ran = d["config"]["gpu_busy_marker_s"] > 0
            assert marker_ran == (on_gpu and bool(extra))
            arrays = {
                p.stem: np.load(p) for p in sorted(out_dir.glob("*.npy"))
            }
            for key in ("desired", "actuated", "oracle"):
                a = arrays[f"{key}_replicas"]
                assert a.dtype == np.float64
                assert a.ndim == 2 and a.shape[1] == 4
            assert arrays["score"][0] == pytest.approx(d["value"], abs=0.006)
            assert sum(a.nbytes for a in arrays.values()) <= 64 * 2**20
            assert (out_dir / "inputs.json").exists()
            dumps.append(arrays)
        assert sources <= ({"reference", "measured"} if on_gpu
                           else {"synthetic"})
        assert dumps[0].keys() == dumps[1].keys()
        assert ("decode_probe_logits" in dumps[0]) == on_gpu
        for key in dumps[0]:
            a, b = dumps[0][key], dumps[1][key]
            assert a.shape == b.shape
            if key != "decode_probe_logits" and "measured" not in sources:
                np.testing.assert_array_equal(a, b)
        if on_gpu:
            a, b = (d["decode_probe_logits"] for d in dumps)
            assert a.dtype == np.float32 and np.isfinite(a).all()
            # bf16 keeps 8 significant bits: ulp(x) = 2^(floor(log2|x|)-7)
            ulp = 2.0 ** (np.floor(np.log2(np.abs(a).max())) - 7)
            np.testing.assert_allclose(a, b, rtol=0, atol=2 * ulp)

    @pytest.mark.timeout(420)
    def test_two_process_gloo(self):
        # the gloo path is the CPU one: hide any GPU from the two ranks,
        # or a host with a single GPU sends both down the NCCL path and
        # rank 1 finds no device of its own
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1",
                   CUDA_VISIBLE_DEVICES="-1")
        out = subprocess.run(
            [
                sys.executable, "-m", "torch.distributed.run",
                "--nnodes=1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", "29531",
                os.path.join(REPO, "bench.py"),
                "--gpus", "2", "--steps", "5", "--warmup", "2",
            ],
            capture_output=True, text=True, timeout=400, cwd=REPO, env=env,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [
            line for line in out.stdout.strip().splitlines()
            if line.startswith("{")
        ]
        assert len(lines) == 1  # only rank 0 prints
        d = json.loads(lines[-1])
        assert d["n_gpus"] == 2
        assert d["config"]["parallelism"] == "dp2"
        assert d["config"]["device"] is None  # ran the CPU (gloo) path
