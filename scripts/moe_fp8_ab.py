#!/usr/bin/env python3
"""Routed-MoE expert MLP with weight-only fp8 (e4m3) expert weights against
bf16 ones on one MI355X, method as in scripts/moe_tiled_ab.py.

    python scripts/moe_fp8_ab.py [OUT_JSON]

Runs two fresh child processes one after another, each under its own
`timeout`, and stops at the first that does not exit 0:

  layer   one Mixtral-8x7B layer's ops.moe_mlp (H=4096, I=14336, E=8, K=2,
          seeded weights, random router logits), variant="stream", with bf16
          weights and with their ops.quantize_moe_weights form, at T = 1 ..
          256 tokens, the two alternating window by window. Per T the JSON
          also keeps the expert-weight bytes each arm has to stream (routed
          experts x 3 H I x element size, counted from the routing), the
          TB/s that is over the median time, and how far the fp8 output is
          from the bf16 one relative to the output's amax: the quantisation
          error, not a kernel error (tests/test_moe_fp8_gpu.py holds the
          kernels to exact and float64 references).
  engine  graphed Mixtral-8x7B ITL (random weights, ctx 512) at B = 1, 8, 64:
          moe_impl="grouped" with bf16 and with fp8 expert weights, and
          moe_impl="auto" (bf16) alongside, alternating window by window.

Every shape is warmed up before it is timed. Every figure is taken WINDOWS
times; the JSON keeps all windows, their median and their max-min spread.
A run without a GPU fails. Writes OUT_JSON (default
profiles/moe_fp8_ab.json).

worker: moe_fp8_ab.py worker <mode> <out_json>
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
TOKENS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
BATCHES = (1, 8, 64)
CTX = 512
ITL_STEPS = 40


def summary(values, unit):
    return {"unit": unit, "windows": values,
            "median": statistics.median(values),
            "spread": max(values) - min(values)}


def time_window(torch, fn):
    """ms per call over one window of >= 0.25 s (at least 5 calls)."""
    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    pilot = run(3) / 3
    n = max(5, int(0.25 / pilot) + 1)
    return run(n) / n * 1e3


def alternate(arms, window):
    """{name: fn} -> {name: [WINDOWS figures]}, one window of each arm in
    turn, every arm warmed first."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    out = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            out[name].append(window(fn))
    return out


def layer_mode(torch, ops, res):
    from wva_amd.calibration.moe_model import MIXTRAL_8X7B as cfg

    H, I, E, K = (cfg.hidden_size, cfg.intermediate_size, cfg.num_experts,
                  cfg.top_k)
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    w_gu = torch.empty(E, 2 * I, H, **bf).normal_(0.0, 0.02, generator=g)
    w_dn = torch.empty(E, H, I, **bf).normal_(0.0, 0.02, generator=g)
    q_gu, s_gu = ops.quantize_moe_weights(w_gu)
    q_dn, s_dn = ops.quantize_moe_weights(w_dn)

    for T in TOKENS:
        x = torch.empty(T, H, **bf).normal_(0.0, 1.0, generator=g)
        logits = torch.empty(T, E, device="cuda").normal_(generator=g)
        arms = {
            "bf16": lambda: ops.moe_mlp(x, logits, w_gu, w_dn, K,
                                        variant="stream"),
            "fp8": lambda: ops.moe_mlp(x, logits, q_gu, q_dn, K,
                                       variant="stream",
                                       w_gate_up_scale=s_gu,
                                       w_down_scale=s_dn),
        }
        got = alternate(arms, lambda fn: time_window(torch, fn))
        routed = int(torch.unique(ops.moe_route(logits, K)[0]).numel())
        out16, out8 = arms["bf16"]().float(), arms["fp8"]().float()
        res[f"T{T}_routed_experts"] = routed
        res[f"T{T}_fp8_vs_bf16_maxdiff_over_amax"] = float(
            (out8 - out16).abs().max() / out16.abs().max())
        for name, values in got.items():
            r = summary(values, "ms")
            res[f"T{T}_{name}_ms"] = r
            nbytes = routed * 3 * H * I * (2 if name == "bf16" else 1)
            res[f"T{T}_{name}_weight_bytes"] = nbytes
            res[f"T{T}_{name}_weight_TBps"] = nbytes / (r["median"] * 1e-3) / 1e12
        print(f"T={T} done", flush=True)


def engine_mode(torch, ops, res):
    from wva_amd.calibration.graph import GraphedDecoder
    from wva_amd.calibration.moe_model import (MIXTRAL_8X7B,
                                               MixtralDecodeModel)

    kw = dict(max_batch=max(BATCHES), max_seq=1024, moe_impl="grouped")
    m16 = MixtralDecodeModel(MIXTRAL_8X7B, **kw)
    m8 = MixtralDecodeModel(MIXTRAL_8X7B, weights_dtype="fp8", **kw)
    res["expert_weight_bytes_bf16"] = sum(
        l.w_gate_up_stacked.nbytes + l.w_down_stacked.nbytes
        for l in m16.layers)
    res["expert_weight_bytes_fp8"] = sum(
        l.w_gate_up_stacked.nbytes + l.w_down_stacked.nbytes
        + l.w_gate_up_scale.nbytes + l.w_down_scale.nbytes
        for l in m8.layers)

    for B in BATCHES:
        tokens = torch.randint(0, MIXTRAL_8X7B.vocab_size, (B,),
                               device="cuda")
        arms = {}
        for name, model, impl in (("grouped_bf16", m16, "grouped"),
                                  ("grouped_fp8", m8, "grouped"),
                                  ("auto_bf16", m16, "auto")):
            model.moe_impl = impl      # frozen into the graph at capture
            model.reset(B, CTX)
            dec = GraphedDecoder(model, B)

            def run(dec=dec):
                dec.reset_to(B, CTX)
                for _ in range(ITL_STEPS):
                    dec.decode_step(tokens)
            arms[name] = run
        m16.moe_impl = "grouped"

        def window(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / ITL_STEPS

        for name, values in alternate(arms, window).items():
            res[f"itl_b{B}_ctx{CTX}_{name}_ms"] = summary(values, "ms")
        print(f"B={B} done", flush=True)


def worker(mode, out_json):
    sys.path.insert(0, REPO)
    import torch
    from wva_amd import ops

    if not torch.cuda.is_available():
        sys.exit("moe_fp8_ab.py measures on a GPU; none found")
    ops._require_ext()
    res = {}
    with torch.no_grad():
        if mode == "layer":
            layer_mode(torch, ops, res)
        elif mode == "engine":
            engine_mode(torch, ops, res)
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
    merged = {"model": "Mixtral-8x7B (random weights)",
              "layer_shape": "H=4096 I=14336 E=8 K=2, random router logits",
              "windows_per_figure": WINDOWS}
    for mode, limit in (("layer", 300), ("engine", 480)):
        part = f"{out_json}.{mode}.part"
        child(mode, limit, part)
        with open(part) as f:
            merged.update(json.load(f))
        os.remove(part)
        with open(out_json, "w") as f:      # keep what is measured so far
            json.dump(merged, f, indent=1)
            f.write("\n")
    for name, r in merged.items():
        if isinstance(r, dict):
            print(f"{name:44s} median {r['median']:10.3f} {r['unit']:3s} "
                  f"spread {r['spread']:8.3f}")
        else:
            print(f"{name:44s} {r}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(*sys.argv[2:4])
    else:
        main(os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else
                             os.path.join(REPO, "profiles",
                                          "moe_fp8_ab.json")))
