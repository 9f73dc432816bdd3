#!/usr/bin/env python3
"""A/B of this checkout's decode attention against another built checkout.

    python scripts/attn_ab.py BASELINE_TREE [OUT_DIR]

BASELINE_TREE is a checkout of the commit to compare against, with its
extension built in-tree. Runs fresh child processes one after another, one
build per process: first the outputs of `auto` and of the pinned v5 kernel
on seeded inputs (bit-identity), then WINDOWS alternating timing windows
per build of `auto` on the attn_bench shapes with a bf16 and an fp8 cache,
each window at least 0.25 s after warm-up. The gate per row: this build's
median minus the baseline's median must not exceed the baseline's own
max-min spread. Stops at the first child that does not exit 0 and writes
OUT_DIR/attn_refactor_ab.txt (profiles/attn_refactor_ab.txt is one such
file).

worker: attn_ab.py worker <tree> <tag> <mode> <outdir>
"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
TREES = {"refactor": REPO}  # "parent" is added from the command line
OUT = "attn_ab_out"

BF16_SHAPES = [(2, 8, 2, 33), (4, 32, 8, 512), (2, 64, 8, 300), (3, 4, 4, 100),
               (2, 8, 1, 2000), (1, 4, 1, 20000)]
FP8_SHAPES = [(4, 32, 8, 512), (2, 64, 8, 300), (2, 8, 1, 2000)]
BENCH_SHAPES = [(64, 32, 8, 512), (64, 32, 8, 2048), (256, 32, 8, 512),
                (8, 64, 8, 4096)]
WINDOWS = 5


def make_inputs(torch, shape, fp8, seed, full_lens):
    batch, hq, hk, ctx = shape
    torch.manual_seed(seed)
    S = max(ctx + 8, 64)
    q = torch.randn(batch, hq, 128, device="cuda", dtype=torch.bfloat16)
    if fp8:
        k = (torch.randn(batch, hk, S, 128, device="cuda") * 0.7).to(
            torch.float8_e4m3fn)
        v = (torch.randn(batch, hk, S, 128, device="cuda") * 0.7).to(
            torch.float8_e4m3fn)
    else:
        k = torch.randn(batch, hk, S, 128, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(batch, hk, S, 128, device="cuda", dtype=torch.bfloat16)
    if full_lens:
        lens = torch.full((batch,), ctx, device="cuda", dtype=torch.int32)
    else:
        lens = torch.randint(1, ctx + 1, (batch,), device="cuda",
                             dtype=torch.int32)
        lens[0] = ctx
    return q, k, v, lens


def worker(tree, tag, mode, outdir):
    sys.path.insert(0, tree)
    import torch
    from wva_amd.ops import _require_ext

    ext = _require_ext()
    assert os.path.dirname(ext.__file__).startswith(tree), ext.__file__
    scale = 128 ** -0.5
    if hasattr(ext, "gqa_decode_attn_v5"):
        v5 = ext.gqa_decode_attn_v5
    else:
        def v5(q, k, v, lens, s):
            return ext.gqa_decode_attn(q, k, v, lens, s, variant="v5")
    os.makedirs(outdir, exist_ok=True)
    if mode == "outputs":
        res = {}
        for fp8, shapes in [(False, BF16_SHAPES), (True, FP8_SHAPES)]:
            for shape in shapes:
                q, k, v, lens = make_inputs(torch, shape, fp8, 11, fp8)
                name = ("fp8" if fp8 else "bf16") + "_" + "x".join(
                    map(str, shape))
                res[name + "_auto"] = ext.gqa_decode_attn(
                    q, k, v, lens, scale).cpu()
                res[name + "_v5"] = v5(q, k, v, lens, scale).cpu()
        torch.cuda.synchronize()
        torch.save(res, os.path.join(outdir, f"outputs_{tag}.pt"))
        print(f"{tag}: saved {len(res)} outputs", flush=True)
    elif mode == "time":
        rows = {}
        for fp8 in (False, True):
            for shape in BENCH_SHAPES:
                batch, hq, hk, ctx = shape
                q = torch.randn(batch, hq, 128, device="cuda",
                                dtype=torch.bfloat16)
                if fp8:
                    k = (torch.randn(batch, hk, ctx, 128, device="cuda")
                         * 0.7).to(torch.float8_e4m3fn)
                    v = (torch.randn(batch, hk, ctx, 128, device="cuda")
                         * 0.7).to(torch.float8_e4m3fn)
                else:
                    k = torch.randn(batch, hk, ctx, 128, device="cuda",
                                    dtype=torch.bfloat16)
                    v = torch.randn(batch, hk, ctx, 128, device="cuda",
                                    dtype=torch.bfloat16)
                lens = torch.full((batch,), ctx, device="cuda",
                                  dtype=torch.int32)

                def run(n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        ext.gqa_decode_attn(q, k, v, lens, scale)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0

                run(200)  # warm-up
                pilot = run(500) / 500
                n = max(500, int(0.35 / pilot) + 1)
                dt = run(n)
                name = ("fp8" if fp8 else "bf16") + "_" + "x".join(
                    map(str, shape))
                rows[name] = {"us": dt / n * 1e6, "n": n, "window_s": dt}
                del q, k, v
        with open(os.path.join(outdir, f"time_{tag}.json"), "w") as f:
            json.dump(rows, f)
        print(f"{tag}: timed {len(rows)} configs", flush=True)


def child(tree_name, tag, mode, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable,
           os.path.abspath(__file__), "worker", TREES[tree_name], tag, mode,
           OUT]
    print("+", " ".join(cmd[4:]), flush=True)
    rc = subprocess.call(cmd)
    if rc != 0:
        print(f"child {tag} {mode} exited {rc}; stopping", flush=True)
        sys.exit(rc if rc > 0 else 1)


def main():
    import torch  # CPU-side only here: no GPU call in the orchestrator

    os.makedirs(OUT, exist_ok=True)
    lines = []
    child("parent", "parent", "outputs", 240)
    child("refactor", "refactor", "outputs", 240)
    a = torch.load(os.path.join(OUT, "outputs_parent.pt"))
    b = torch.load(os.path.join(OUT, "outputs_refactor.pt"))
    lines.append("Bit-identity, refactor vs parent build (same seeded inputs, "
                 "one fresh process per build)")
    lines.append(f"{'case':34s} {'max|diff|':>10s} equal")
    worst = 0.0
    for name in sorted(a):
        d = (a[name].float() - b[name].float()).abs().max().item()
        finite = bool(torch.isfinite(a[name].float()).all())
        worst = max(worst, d)
        lines.append(f"{name:34s} {d:10.3g} {torch.equal(a[name], b[name])}"
                     + ("" if finite else "  (non-finite in parent!)"))
    lines.append(f"max abs diff over all cases: {worst:g}")
    lines.append("")
    with open(os.path.join(OUT, "attn_refactor_ab.txt"),
              "w") as f:
        f.write("\n".join(lines) + "\n")

    for w in range(WINDOWS):
        child("parent", f"parent_w{w}", "time", 300)
        child("refactor", f"refactor_w{w}", "time", 300)
    t = {}
    for build in ("parent", "refactor"):
        for w in range(WINDOWS):
            with open(os.path.join(OUT, f"time_{build}_w{w}.json")) as f:
                for name, r in json.load(f).items():
                    t.setdefault(name, {}).setdefault(build, []).append(r)
    lines.append("Speed, `auto` dispatch, us per call; builds alternated in "
                 f"fresh processes, {WINDOWS} windows each, each window "
                 ">= 0.25 s after warm-up")
    lines.append("gate: median(refactor) - median(parent) <= "
                 "max-min spread of the parent's windows")
    ok_all = True
    for name, r in t.items():
        p = [x["us"] for x in r["parent"]]
        n = [x["us"] for x in r["refactor"]]
        mp, mn = statistics.median(p), statistics.median(n)
        spread = max(p) - min(p)
        ok = (mn - mp) <= spread
        ok_all &= ok
        lines.append(
            f"{name:22s} parent {' '.join('%8.2f' % x for x in p)} "
            f"med {mp:8.2f} spread {spread:6.2f} | refactor "
            f"{' '.join('%8.2f' % x for x in n)} med {mn:8.2f} "
            f"spread {max(n) - min(n):6.2f} | delta {mn - mp:+7.2f} "
            f"{'ok' if ok else 'SLOWER'}  (min window "
            f"{min(x['window_s'] for x in r['parent'] + r['refactor']):.2f} s)")
    lines.append(f"speed gate: {'pass' if ok_all else 'FAIL'}")
    with open(os.path.join(OUT, "attn_refactor_ab.txt"),
              "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(*sys.argv[2:6])
    elif len(sys.argv) < 2:
        sys.exit(__doc__)
    else:
        TREES["parent"] = os.path.abspath(sys.argv[1])
        if len(sys.argv) > 2:
            OUT = sys.argv[2]
        OUT = os.path.abspath(OUT)
        main()
