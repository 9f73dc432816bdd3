#!/usr/bin/env python3
"""Ragged chunked prefill on one MI355X: the split-KV sweep behind
extend_attn_ragged_num_splits, extend_attn_ragged against extend_attn, and
ragged_step against the mixed_step calls it replaces.

    python scripts/ragged_extend_ab.py [OUT_JSON]

Runs two fresh child processes one after another, each under its own
`timeout`, and stops at the first that does not exit 0:

  kernel  Hq=32, Hk=8, B=1, bf16 cache, seeded inputs.
          sweep: extend_attn_ragged with num_splits forced to each of SPLITS
            at prefix 8192 with C = 64, 256, 512 and at prefix 0 with
            C = 2048, the split counts alternating window by window;
          weak shape (prefix 8192, C=64) and prefix 0, C=2048: extend_attn
            against extend_attn_ragged at the heuristic's count, alternating
            window by window. The ragged arm is timed twice: the public op
            (which also forms q_starts with two small device kernels) and
            the binding with q_starts precomputed (zero-fill + attention +
            merge only);
  engine  Llama-3-8B bf16, 32 decode rows at ctx 512 plus chunks of 512, 64
          and 17 tokens behind prefixes of 512: one ragged_step, against
          the same chunks as three calls (mixed_step with the 512-token
          chunk, then prefill_chunk of 64 and of 17, i.e. three passes over
          the weights) and against one mixed_step with all three padded to
          512; the three arms alternate window by window.

Every shape is warmed up before it is timed. Every figure is taken WINDOWS
times; the JSON keeps all windows, their median and their max-min spread.
A run without a GPU fails. Writes OUT_JSON (default
profiles/ragged_extend_ab.json).

worker: ragged_extend_ab.py worker <mode> <out_json>
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
HQ, HK = 32, 8
LONG_PREFIX = 8192
SPLITS = (1, 2, 4, 8, 16, 24)
SWEEP_SHAPES = ((LONG_PREFIX, 64), (LONG_PREFIX, 256), (LONG_PREFIX, 512),
                (0, 2048))
AB_SHAPES = ((LONG_PREFIX, 64), (0, 2048))
DECODE_BATCH, CTX = 32, 512
CHUNK_LENS = (512, 64, 17)


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


def alternate(torch, arms):
    """{name: fn} -> {name: [WINDOWS figures]}, one window of each arm in
    turn."""
    out = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            out[name].append(time_kernel(torch, fn))
    return out


def kernel_mode(torch, ops, res):
    ext = ops._require_ext()
    scale = 128 ** -0.5
    torch.manual_seed(0)

    def case(prefix, chunk):
        S = prefix + chunk
        bf = dict(device="cuda", dtype=torch.bfloat16)
        i32 = dict(device="cuda", dtype=torch.int32)
        return dict(q=torch.randn(chunk, HQ, 128, **bf),
                    k=torch.randn(1, HK, S, 128, **bf),
                    v=torch.randn(1, HK, S, 128, **bf),
                    P=torch.full((1,), prefix, **i32),
                    L=torch.full((1,), chunk, **i32),
                    Q=torch.zeros(1, **i32), chunk=chunk, S=S)

    def ragged(c, n):
        return lambda: ops.extend_attn_ragged(
            c["q"], c["k"], c["v"], c["P"], c["L"], c["chunk"], scale, n)

    for prefix, chunk in SWEEP_SHAPES:
        c = case(prefix, chunk)
        got = alternate(torch, {n: ragged(c, n) for n in SPLITS})
        for n in SPLITS:
            res[f"sweep_P{prefix}_C{chunk}_splits{n}_us"] = summary(
                got[n], "us")

    for prefix, chunk in AB_SHAPES:
        c = case(prefix, chunk)
        n = ops.extend_attn_ragged_num_splits(1, HQ, chunk, c["S"])
        res[f"heuristic_P{prefix}_C{chunk}_splits"] = n
        got = alternate(torch, {
            "extend_attn": lambda: ops.extend_attn(
                c["q"], c["k"], c["v"], c["P"], chunk, scale),
            "ragged_op": ragged(c, None),
            "ragged_binding": lambda: ext.extend_attn_ragged(
                c["q"], c["k"], c["v"], c["P"], c["Q"], c["L"], chunk, scale,
                n),
        })
        if n == 1:  # the unsplit path promises the bits of extend_attn
            same = torch.equal(
                ops.extend_attn(c["q"], c["k"], c["v"], c["P"], chunk, scale),
                ragged(c, None)())
            res[f"ab_P{prefix}_C{chunk}_bit_equal"] = bool(same)
        for name, values in got.items():
            res[f"ab_P{prefix}_C{chunk}_{name}_us"] = summary(values, "us")


def engine_mode(torch, res):
    from wva_amd.calibration.model import LLAMA_3_8B, LlamaDecodeModel

    Bp, C = len(CHUNK_LENS), max(CHUNK_LENS)
    m = LlamaDecodeModel(LLAMA_3_8B, max_batch=DECODE_BATCH + Bp,
                         max_seq=CTX + C + 64)
    m.reset(DECODE_BATCH + Bp, CTX)
    lens0 = m.context_lens.clone()
    g = torch.Generator(device="cuda").manual_seed(0)

    def toks(*shape):
        return torch.randint(0, m.cfg.vocab_size, shape, device="cuda",
                             generator=g)

    dec = toks(DECODE_BATCH)
    packed = toks(sum(CHUNK_LENS))
    c_lens = torch.tensor(CHUNK_LENS, dtype=torch.int32, device="cuda")
    singles = [toks(1, n) for n in CHUNK_LENS]
    padded = toks(Bp, C)

    def three_calls():
        m.mixed_step(dec, singles[0])
        m.prefill_chunk(singles[1])
        m.prefill_chunk(singles[2])

    arms = {
        "ragged_step": lambda: m.ragged_step(dec, packed, c_lens, C),
        "three_calls": three_calls,
        "mixed_step_padded": lambda: m.mixed_step(dec, padded),
    }

    def window(fn, iters=8):
        """median wall ms of one iteration; context_lens put back first"""
        times = []
        for _ in range(iters):
            m.context_lens.copy_(lens0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1000.0)
        return statistics.median(times)

    for fn in arms.values():          # warm every shape
        window(fn, iters=3)
    out = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            out[name].append(window(fn))
    tag = "x".join(str(n) for n in CHUNK_LENS)
    for name, values in out.items():
        res[f"itl_b{DECODE_BATCH}_ctx{CTX}_chunks{tag}_{name}_ms"] = summary(
            values, "ms")


def worker(mode, out_json):
    sys.path.insert(0, REPO)
    import torch
    from wva_amd import ops

    if not torch.cuda.is_available():
        sys.exit("ragged_extend_ab.py measures on a GPU; none found")
    ops._require_ext()
    res = {}
    if mode == "kernel":
        kernel_mode(torch, ops, res)
    elif mode == "engine":
        engine_mode(torch, res)
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
              "attention_shape": f"Hq={HQ} Hk={HK} B=1 bf16 cache",
              "windows_per_figure": WINDOWS}
    for mode, limit in (("kernel", 300), ("engine", 240)):
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
            print(f"{name:52s} median {r['median']:10.2f} {r['unit']:3s} "
                  f"spread {r['spread']:8.2f}")
        else:
            print(f"{name:52s} {r}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(*sys.argv[2:4])
    else:
        main(os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else
                             os.path.join(REPO, "profiles",
                                          "ragged_extend_ab.json")))
