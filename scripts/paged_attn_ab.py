#!/usr/bin/env python3
"""A/B of the paged KV cache against the contiguous one, same build.

    python scripts/paged_attn_ab.py [OUT_JSON]

Two measurements, every configuration in a fresh child process:

  * decode attention, us per call (launch + kernel + merge, host clock
    around a device synchronise): the contiguous kernel against the paged
    kernel at block sizes 16 and 64 on the same K/V rows, scattered over a
    randomly permuted pool. Shapes: the BENCH_SHAPES of attn_ab.py plus
    (1, 32, 8, 131072); bf16 and fp8; `auto` and the pinned v4 and v5. One
    child per (dtype, shape); inside it the nine arms run in WINDOWS
    alternating windows, and every pinned paged output is checked bit-equal
    to its contiguous counterpart first.
  * step level: measure_itl of Llama-3-8B at b=64, ctx=512, contiguous
    against paged (16), eager and graphed; one child per layout per window,
    layouts alternating.

Medians and max-min spreads go to OUT_JSON (default
profiles/paged_attn_ab.json). There is no pass/fail ratio: the file records
what pages cost. Stops at the first child that does not exit 0.

worker: paged_attn_ab.py worker <mode> <spec-json> <out-file>
"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from attn_ab import BENCH_SHAPES  # noqa: E402

SHAPES = BENCH_SHAPES + [(1, 32, 8, 131072)]
BLOCK_SIZES = (16, 64)
VARIANTS = ("auto", "v4", "v5")
WINDOWS = 3
WINDOW_S = 0.12
ITL_WINDOWS = 2
ITL = {"batch": 64, "context_len": 512, "max_seq": 1024, "iters": 20}


def attn_worker(spec, out_file):
    sys.path.insert(0, REPO)
    import torch
    from wva_amd import ops

    batch, hq, hk, ctx = spec["shape"]
    fp8 = spec["fp8"]
    scale = 128 ** -0.5
    torch.manual_seed(1)
    q = torch.randn(batch, hq, 128, device="cuda", dtype=torch.bfloat16)
    lens = torch.full((batch,), ctx, device="cuda", dtype=torch.int32)

    def cache():
        t = torch.randn(batch, hk, ctx, 128, device="cuda",
                        dtype=torch.bfloat16)
        return (t * 0.7).to(torch.float8_e4m3fn) if fp8 else t

    k, v = cache(), cache()
    splits = ops.gqa_decode_num_splits(batch, hk, ctx)

    def pool_of(t, bs, perm):
        """Page i of the row-major (b, block) list goes to pool[perm[i]]."""
        raw = t.view(torch.uint8) if fp8 else t
        nblk = ctx // bs
        pages = (raw.reshape(batch, hk, nblk, bs, 128).permute(0, 2, 1, 3, 4)
                 .reshape(batch * nblk, hk, bs, 128))
        pool = torch.empty(pages.shape, dtype=pages.dtype, device="cuda")
        pool[perm] = pages
        return pool.view(t.dtype)

    arms = {}
    for variant in VARIANTS:
        arms[f"contiguous_{variant}"] = (
            lambda variant=variant: ops.gqa_decode_attn(
                q, k, v, lens, scale, variant=variant))
    for bs in BLOCK_SIZES:
        n = batch * (ctx // bs)
        perm = torch.randperm(n, device="cuda")
        tables = perm.reshape(batch, ctx // bs).to(torch.int32).contiguous()
        kp, vp = pool_of(k, bs, perm), pool_of(v, bs, perm)
        for variant in VARIANTS:
            arms[f"paged{bs}_{variant}"] = (
                lambda variant=variant, kp=kp, vp=vp, tables=tables:
                ops.paged_decode_attn(q, kp, vp, tables, lens, scale, splits,
                                      variant=variant))
    for name, fn in arms.items():  # same rows, same splits: same bits
        ref = arms["contiguous_" + name.split("_")[1]]
        assert torch.equal(fn(), ref()), name

    def run(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    counts = {}
    for name, fn in arms.items():
        run(fn, 30)  # warm-up
        pilot = run(fn, 50) / 50
        counts[name] = max(50, int(WINDOW_S / pilot) + 1)
    rows = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, fn in arms.items():
            rows[name].append(run(fn, counts[name]) / counts[name] * 1e6)
    with open(out_file, "w") as f:
        json.dump({"splits": splits, "us": rows, "calls": counts}, f)
    print(f"timed {spec}", flush=True)


def itl_worker(spec, out_file):
    sys.path.insert(0, REPO)
    import torch  # noqa: F401
    from wva_amd.calibration.itl_benchmark import measure_itl
    from wva_amd.calibration.model import LLAMA_3_8B, LlamaDecodeModel

    kw = {}
    if spec["layout"] == "paged":
        kw = dict(kv_layout="paged", block_size=16)
    model = LlamaDecodeModel(LLAMA_3_8B, max_batch=ITL["batch"],
                             max_seq=ITL["max_seq"], **kw)
    res = {}
    for graph in (False, True):
        res["graphed" if graph else "eager"] = measure_itl(
            model, ITL["batch"], ITL["context_len"], iters=ITL["iters"],
            use_graph=graph)
    with open(out_file, "w") as f:
        json.dump(res, f)
    print(f"itl {spec}: {res}", flush=True)


def child(mode, spec, out_file, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable,
           os.path.abspath(__file__), "worker", mode, json.dumps(spec),
           out_file]
    print("+", mode, json.dumps(spec), flush=True)
    rc = subprocess.call(cmd)
    if rc != 0:
        print(f"child {mode} {spec} exited {rc}; stopping", flush=True)
        sys.exit(rc if rc > 0 else 1)
    with open(out_file) as f:
        return json.load(f)


def summary(values):
    return {"median": round(statistics.median(values), 3),
            "spread": round(max(values) - min(values), 3),
            "windows": [round(x, 3) for x in values]}


def main(out_json):
    os.makedirs(os.path.dirname(out_json), exist_ok=True)
    tmp = out_json + ".child"
    result = {
        "method": (
            f"us per call = host clock around a synchronise, {WINDOWS} "
            f"alternating windows of >= {WINDOW_S} s per arm inside one "
            "fresh process per (dtype, shape); itl = measure_itl median of "
            f"{ITL['iters']} steps, one fresh process per layout per "
            f"window, {ITL_WINDOWS} windows; spread = max - min of the "
            "windows; ratio = paged median / contiguous median"),
        "attention_us_per_call": {}, "itl_ms": {}}
    for fp8 in (False, True):
        for shape in SHAPES:
            r = child("attn", {"shape": list(shape), "fp8": fp8}, tmp, 300)
            name = ("fp8" if fp8 else "bf16") + "_" + "x".join(map(str, shape))
            row = {"splits": r["splits"]}
            for arm, us in r["us"].items():
                row[arm] = summary(us)
            for bs in BLOCK_SIZES:
                for variant in VARIANTS:
                    row[f"ratio_paged{bs}_{variant}"] = round(
                        row[f"paged{bs}_{variant}"]["median"]
                        / row[f"contiguous_{variant}"]["median"], 4)
            result["attention_us_per_call"][name] = row
            print(name, {k: v for k, v in row.items()
                         if k.startswith("ratio")}, flush=True)
    itl = {}
    for _ in range(ITL_WINDOWS):
        for layout in ("contiguous", "paged"):
            r = child("itl", {"layout": layout}, tmp, 400)
            for mode, ms in r.items():
                itl.setdefault(f"{layout}_{mode}", []).append(ms)
    result["itl_ms"] = {k: summary(v) for k, v in itl.items()}
    result["itl_ms"]["config"] = dict(ITL, model="Llama-3-8B", block_size=16)
    for mode in ("eager", "graphed"):
        result["itl_ms"][f"ratio_paged_{mode}"] = round(
            result["itl_ms"][f"paged_{mode}"]["median"]
            / result["itl_ms"][f"contiguous_{mode}"]["median"], 4)
    os.remove(tmp)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["itl_ms"], indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        mode, spec, out_file = sys.argv[2], json.loads(sys.argv[3]), sys.argv[4]
        (attn_worker if mode == "attn" else itl_worker)(spec, out_file)
    else:
        main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1
             else os.path.join(REPO, "profiles", "paged_attn_ab.json"))
