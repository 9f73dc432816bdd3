#!/usr/bin/env python3
"""Routed-MoE expert MLP at prefill scale on one MI355X: the tiled grouped
GEMMs (variant="tiled") against the streaming ones (variant="stream") and
the engine's sparse path, the measurement behind moe_use_tiled.

    python scripts/moe_tiled_ab.py [OUT_JSON]

Runs two fresh child processes one after another, each under its own
`timeout`, and stops at the first that does not exit 0:

  layer   one Mixtral-8x7B layer's expert MLP (H=4096, I=14336, E=8, K=2,
          seeded weights, random router logits) at T = 256 .. 4096 tokens.
          Arms, alternating window by window: ops.moe_mlp(variant="stream"),
          ops.moe_mlp(variant="tiled"), and MixtralDecodeModel's
          _moe_mlp_sparse (with the top-k and softmax the engine runs in
          front of it) on the same inputs. Before the timing, at every T,
          the two variants' gate_up outputs are held to the oracle's
          gate_up bound and their down outputs (on the same act) to its
          down bound, both against a float64 reference computed on the
          GPU with the formulas of tests/moe_oracle.py; the JSON keeps the
          worst error/bound ratio of each arm and how far the arms are
          apart in units of the bound.
  engine  one full prefill, B=1, S=2048, Mixtral-8x7B with random weights,
          under moe_impl="sparse" and moe_impl="grouped" of one model, the
          two alternating window by window.

Every shape is warmed up before it is timed. Every figure is taken WINDOWS
times; the JSON keeps all windows, their median and their max-min spread.
A run without a GPU fails. Writes OUT_JSON (default
profiles/moe_tiled_ab.json).

worker: moe_tiled_ab.py worker <mode> <out_json>
"""
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
WINDOWS = 5
TOKENS = (256, 512, 1024, 2048, 4096)
PREFILL_S = 2048


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


def alternate(torch, arms):
    """{name: fn} -> {name: [WINDOWS figures]}, one window of each arm in
    turn, every arm warmed first."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    out = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            out[name].append(time_window(torch, fn))
    return out


def check_outputs(torch, ops, x, logits, w_gu, w_dn, K, res, tag):
    """Both variants against float64 on the GPU, bounds as in
    tests/moe_oracle.py (gate_up_bound, down_bound)."""
    H, I = x.shape[1], w_dn.shape[2]
    _, topk_w, offsets, slots = ops.moe_route(logits, K)
    offs = offsets.tolist()
    tokens = torch.div(slots.long(), K, rounding_mode="floor")
    acts = {v: ops.moe_gate_up_swiglu(x, w_gu, offsets, slots, K, variant=v)
            for v in ("stream", "tiled")}
    outs = {v: ops.moe_down_combine(acts["stream"], w_dn, topk_w, offsets,
                                    slots, variant=v)
            for v in ("stream", "tiled")}
    xs = x.double()[tokens]
    a = acts["stream"].double()
    TK = slots.numel()
    gu = torch.zeros(TK, 2 * I, dtype=torch.float64, device=x.device)
    ab = torch.zeros_like(gu)
    y = torch.zeros(TK, H, dtype=torch.float64, device=x.device)
    ya = torch.zeros_like(y)
    for e in range(w_gu.shape[0]):
        lo, hi = offs[e], offs[e + 1]
        if hi > lo:
            we = w_gu[e].double()
            gu[lo:hi] = xs[lo:hi] @ we.t()
            ab[lo:hi] = xs[lo:hi].abs() @ we.abs().t()
            wd = w_dn[e].double()
            y[lo:hi] = a[lo:hi] @ wd.t()
            ya[lo:hi] = a[lo:hi].abs() @ wd.abs().t()
    g, u, absg, absu = gu[:, :I], gu[:, I:], ab[:, :I], ab[:, I:]
    silu = g / (1 + torch.exp(-g))
    ref = silu * u
    dg = (H + 16) * 2.0 ** -23 * absg
    du = (H + 16) * 2.0 ** -23 * absu
    bound = ((2.0 ** -8 + 2.0 ** -12) * ref.abs()
             + 1.1 * dg * (u.abs() + du) + silu.abs() * du)
    ok = bound > 0
    for v, act in acts.items():
        res[f"{tag}_gate_up_{v}_err_over_bound"] = float(
            ((act.double() - ref).abs()[ok] / bound[ok]).max())
    res[f"{tag}_gate_up_arms_apart_over_bound"] = float(
        ((acts["tiled"].double() - acts["stream"].double()).abs()[ok]
         / bound[ok]).max())
    pos = torch.argsort(slots.long())
    tw = topk_w.double()[:, :, None]
    T = x.shape[0]
    dref = (y[pos].reshape(T, K, H) * tw).sum(1)
    dabs = (ya[pos].reshape(T, K, H) * tw.abs()).sum(1)
    dbound = 2.0 ** -8 * dref.abs() + (I + 16 + K) * 2.0 ** -23 * dabs
    ok = dbound > 0
    for v, out in outs.items():
        res[f"{tag}_down_{v}_err_over_bound"] = float(
            ((out.double() - dref).abs()[ok] / dbound[ok]).max())
    res[f"{tag}_down_arms_apart_over_bound"] = float(
        ((outs["tiled"].double() - outs["stream"].double()).abs()[ok]
         / dbound[ok]).max())


def layer_mode(torch, ops, res):
    from wva_amd.calibration.moe_model import (MIXTRAL_8X7B,
                                               MixtralDecodeModel)

    cfg = MIXTRAL_8X7B
    H, I, E, K = (cfg.hidden_size, cfg.intermediate_size, cfg.num_experts,
                  cfg.top_k)
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    w_gu = torch.empty(E, 2 * I, H, **bf).normal_(0.0, 0.02, generator=g)
    w_dn = torch.empty(E, H, I, **bf).normal_(0.0, 0.02, generator=g)
    engine = SimpleNamespace(cfg=cfg)
    layer = SimpleNamespace(w_gate_up=list(w_gu), w_down=list(w_dn))

    for T in TOKENS:
        x = torch.empty(T, H, **bf).normal_(0.0, 1.0, generator=g)
        logits = torch.empty(T, E, device="cuda").normal_(generator=g)
        check_outputs(torch, ops, x, logits, w_gu, w_dn, K, res, f"T{T}")

        def sparse():
            wts, sel = torch.topk(logits, K, dim=-1)
            wts = torch.softmax(wts, dim=-1).to(x.dtype)
            return MixtralDecodeModel._moe_mlp_sparse(engine, layer, x, wts,
                                                      sel)

        got = alternate(torch, {
            "stream": lambda: ops.moe_mlp(x, logits, w_gu, w_dn, K,
                                          variant="stream"),
            "tiled": lambda: ops.moe_mlp(x, logits, w_gu, w_dn, K,
                                         variant="tiled"),
            "sparse": sparse,
        })
        for name, values in got.items():
            res[f"T{T}_{name}_ms"] = summary(values, "ms")
        res[f"T{T}_rule"] = ops.moe_variant(T, K, E)
        print(f"T={T} done", flush=True)


def engine_mode(torch, ops, res):
    from wva_amd.calibration.moe_model import (MIXTRAL_8X7B,
                                               MixtralDecodeModel)

    m = MixtralDecodeModel(MIXTRAL_8X7B, max_batch=1, max_seq=PREFILL_S)
    tokens = torch.randint(0, m.cfg.vocab_size, (1, PREFILL_S), device="cuda")

    def arm(impl):
        def run():
            m.moe_impl = impl
            m.prefill(tokens)
        return run

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    arms = {"sparse": arm("sparse"), "grouped": arm("grouped")}
    for fn in arms.values():          # warm every shape
        fn()
        fn()
    out = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            out[name].append(window(fn))
    for name, values in out.items():
        res[f"prefill_b1_s{PREFILL_S}_{name}_ms"] = summary(values, "ms")
    res["prefill_grouped_variant"] = ops.moe_variant(
        PREFILL_S, m.cfg.top_k, m.cfg.num_experts)


def worker(mode, out_json):
    sys.path.insert(0, REPO)
    import torch
    from wva_amd import ops

    if not torch.cuda.is_available():
        sys.exit("moe_tiled_ab.py measures on a GPU; none found")
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
    merged = {"model": "Mixtral-8x7B bf16 (random weights)",
              "layer_shape": "H=4096 I=14336 E=8 K=2, random router logits",
              "windows_per_figure": WINDOWS}
    for mode, limit in (("layer", 300), ("engine", 420)):
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
                                          "moe_tiled_ab.json")))
