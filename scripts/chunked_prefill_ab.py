#!/usr/bin/env python3
"""Chunked prefill on Llama-3-8B bf16: what it costs against one-shot prefill.

    python scripts/chunked_prefill_ab.py [OUT_JSON]

Runs three fresh child processes one after another, each under its own
`timeout`, and stops at the first that does not exit 0:

  engine  one-shot prefill tokens/s at B=1, S=2048 (measure_prefill_tps, the
          baseline) and chunked prefill of the same prompt with chunks of
          256, 512 and 1024 (measure_chunked_prefill_tps);
  kernel  kernel-only time of extend_attn at prefix 0, C=2048 against
          prefill_attn at S=2048, and of extend_attn at prefix 8192 with
          C=512 and C=64 (Hq=32, Hk=8, B=1, bf16 cache);
  mixed   decode ITL at batch 32, ctx 512, with and without a 512-token
          chunk riding along (measure_mixed_itl).

Every figure is taken WINDOWS times; the JSON keeps all windows, their
median and their max-min spread. Writes OUT_JSON (default
profiles/chunked_prefill_ab.json).

worker: chunked_prefill_ab.py worker <mode> <out_json>
"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
WINDOWS = 5
SEQ = 2048
CHUNKS = (256, 512, 1024)
LONG_PREFIX = 8192
HQ, HK = 32, 8


def summary(values, unit):
    return {"unit": unit, "windows": values,
            "median": statistics.median(values),
            "spread": max(values) - min(values)}


def time_kernel(torch, fn):
    """us per call: warm-up, a pilot, then one window of >= 0.25 s."""
    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    run(20)
    pilot = run(50) / 50
    n = max(50, int(0.25 / pilot) + 1)
    return run(n) / n * 1e6


def worker(mode, out_json):
    sys.path.insert(0, REPO)
    import torch
    from wva_amd import ops
    from wva_amd.calibration import itl_benchmark as ib
    from wva_amd.calibration.model import LLAMA_3_8B, LlamaDecodeModel

    ops._require_ext()
    res = {}
    if mode == "engine":
        m = LlamaDecodeModel(LLAMA_3_8B, max_batch=1, max_seq=SEQ)
        res["prefill_one_shot_tps"] = summary(
            [ib.measure_prefill_tps(m, batch=1, seq=SEQ, iters=3)
             for _ in range(WINDOWS)], "tokens/s")
        for c in CHUNKS:
            res[f"prefill_chunk{c}_tps"] = summary(
                [ib.measure_chunked_prefill_tps(m, 1, SEQ, c, iters=3)
                 for _ in range(WINDOWS)], "tokens/s")
    elif mode == "kernel":
        scale = 128 ** -0.5
        torch.manual_seed(0)

        def case(prefix, chunk):
            S = prefix + chunk
            q = torch.randn(chunk, HQ, 128, device="cuda",
                            dtype=torch.bfloat16)
            k = torch.randn(1, HK, S, 128, device="cuda",
                            dtype=torch.bfloat16)
            v = torch.randn(1, HK, S, 128, device="cuda",
                            dtype=torch.bfloat16)
            P = torch.full((1,), prefix, device="cuda", dtype=torch.int32)
            return q, k, v, P

        q, k, v, P = case(0, SEQ)
        # the two prefix-0 arms alternate window by window
        one, ext = [], []
        for _ in range(WINDOWS):
            one.append(time_kernel(
                torch, lambda: ops.prefill_attn(q, k, v, 1, SEQ, scale)))
            ext.append(time_kernel(
                torch, lambda: ops.extend_attn(q, k, v, P, SEQ, scale)))
        res[f"prefill_attn_S{SEQ}_us"] = summary(one, "us")
        res[f"extend_attn_P0_C{SEQ}_us"] = summary(ext, "us")
        for chunk in (512, 64):
            q, k, v, P = case(LONG_PREFIX, chunk)
            res[f"extend_attn_P{LONG_PREFIX}_C{chunk}_us"] = summary(
                [time_kernel(
                    torch, lambda: ops.extend_attn(q, k, v, P, chunk, scale))
                 for _ in range(WINDOWS)], "us")
    elif mode == "mixed":
        m = LlamaDecodeModel(LLAMA_3_8B, max_batch=33, max_seq=1088)
        for chunk in (0, 512):
            res[f"itl_b32_ctx512_chunk{chunk}_ms"] = summary(
                [ib.measure_mixed_itl(m, 32, 512, chunk, iters=8)
                 for _ in range(WINDOWS)], "ms")
    else:
        sys.exit(f"unknown mode {mode}")
    res["device"] = torch.cuda.get_device_name(0)
    with open(out_json, "w") as f:
        json.dump(res, f)
    print(f"{mode}: {len(res) - 1} figures", flush=True)


def child(mode, limit, part):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable,
           os.path.abspath(__file__), "worker", mode, part]
    print("+", " ".join(cmd[4:]), flush=True)
    rc = subprocess.call(cmd)
    if rc != 0:
        print(f"child {mode} exited {rc}; stopping", flush=True)
        sys.exit(rc if rc > 0 else 1)


def main(out_json):
    os.makedirs(os.path.dirname(out_json), exist_ok=True)
    merged = {"model": "Llama-3-8B bf16 (random weights)",
              "windows_per_figure": WINDOWS}
    for mode, limit in (("engine", 240), ("kernel", 180), ("mixed", 180)):
        part = f"{out_json}.{mode}.part"
        child(mode, limit, part)
        with open(part) as f:
            merged.update(json.load(f))
        os.remove(part)
    with open(out_json, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    for name, r in merged.items():
        if isinstance(r, dict):
            print(f"{name:34s} median {r['median']:12.2f} {r['unit']:9s} "
                  f"spread {r['spread']:10.2f}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(*sys.argv[2:4])
    else:
        main(os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else
                             os.path.join(REPO, "profiles",
                                          "chunked_prefill_ab.json")))
