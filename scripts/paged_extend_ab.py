#!/usr/bin/env python3
"""Paged chunked prefill on one MI355X, against the contiguous arms of the
same run.

    python scripts/paged_extend_ab.py [OUT_JSON]

Three fresh child processes one after another, each under its own `timeout`;
the first that does not exit 0 stops the run. In each, the arms alternate
window by window (timing helpers of ragged_extend_ab.py):

  attn    extend_attn_ragged_paged at block 16 and 64 against
          extend_attn_ragged on the same rows under a random page
          permutation, at the same split count (the heuristic's; the outputs
          are also compared bit for bit). Hq=32, Hk=8, B=1, bf16 and fp8
          caches; prefix 8192 with C=64 and C=512, prefix 0 with C=2048.
  append  rope_append_kv_chunk_paged (block 16, bf16) against the torch
          sequence it replaces per layer: blocks.prefill_qkv plus the two
          indexed writes of ragged_step into a contiguous slab. One chunk of
          512 rows, and chunks of 64 + 17 rows, behind prefixes of 512.
  engine  Llama-3-8B bf16: paged_ragged_step (block 16) against contiguous
          ragged_step, 32 decode rows at ctx 512 plus chunks of 512, 64 and
          17 tokens behind prefixes of 512.

Every figure is taken WINDOWS times; the JSON keeps all windows, their median
and their max-min spread. Nothing here is asserted by a test. A run without a
GPU fails. Writes OUT_JSON (default profiles/paged_extend_ab.json).

worker: paged_extend_ab.py worker <mode> <out_json>
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
from ragged_extend_ab import WINDOWS, alternate, summary  # noqa: E402

HQ, HK, D = 32, 8, 128
ATTN_SHAPES = ((8192, 64), (8192, 512), (0, 2048))
APPEND_CHUNKS = ((512,), (64, 17))
DECODE_BATCH, CTX = 32, 512
CHUNK_LENS = (512, 64, 17)


def to_pool(torch, cache, bs, perm):
    """[1, Hk, S, D] -> pool [S / bs, Hk, bs, D] with block i at page
    perm[i]; e4m3 moves as bytes."""
    raw = cache.view(torch.uint8) if cache.dtype != torch.bfloat16 else cache
    _, Hk, S, d = raw.shape
    pages = raw[0].reshape(Hk, S // bs, bs, d).permute(1, 0, 2, 3)
    pool = torch.empty_like(pages.contiguous())
    pool[perm.long()] = pages
    return pool.view(cache.dtype)


def attn_mode(torch, ops, res):
    scale = D ** -0.5
    torch.manual_seed(0)
    i32 = dict(device="cuda", dtype=torch.int32)
    for name, dtype in (("bf16", torch.bfloat16), ("fp8", torch.float8_e4m3fn)):
        for prefix, chunk in ATTN_SHAPES:
            S = prefix + chunk
            q = torch.randn(chunk, HQ, D, device="cuda", dtype=torch.bfloat16)
            k, v = (torch.randn(1, HK, S, D, device="cuda",
                                dtype=torch.bfloat16).to(dtype)
                    for _ in range(2))
            P, L = torch.full((1,), prefix, **i32), torch.full((1,), chunk, **i32)
            n = ops.extend_attn_ragged_num_splits(1, HQ, chunk, S)
            arms = {"contiguous": lambda: ops.extend_attn_ragged(
                q, k, v, P, L, chunk, scale, n)}
            tag = f"attn_{name}_P{prefix}_C{chunk}"
            res[f"{tag}_splits"] = n
            for bs in (16, 64):
                perm = torch.randperm(S // bs, device="cuda").to(torch.int32)
                kp, vp = to_pool(torch, k, bs, perm), to_pool(torch, v, bs, perm)
                arms[f"paged{bs}"] = (
                    lambda kp=kp, vp=vp, t=perm[None].contiguous():
                    ops.extend_attn_ragged_paged(q, kp, vp, t, P, L, chunk,
                                                 scale, n))
                res[f"{tag}_paged{bs}_bit_equal"] = bool(torch.equal(
                    arms[f"paged{bs}"](), arms["contiguous"]()))
            for arm, values in alternate(torch, arms).items():
                res[f"{tag}_{arm}_us"] = summary(values, "us")


def append_mode(torch, ops, res):
    from wva_amd.calibration import blocks
    from wva_amd.calibration.model import LLAMA_3_8B as cfg

    torch.manual_seed(0)
    bs, S = 16, CTX + 512
    for lens in APPEND_CHUNKS:
        B, T = len(lens), sum(lens)
        bf = dict(device="cuda", dtype=torch.bfloat16)
        qkv = torch.randn(T, cfg.q_size + 2 * cfg.kv_size, **bf)
        kc, vc = (torch.zeros(B, HK, S, D, **bf) for _ in range(2))
        kp, vp = (torch.zeros(B * S // bs, HK, bs, D, **bf) for _ in range(2))
        tables = torch.randperm(B * S // bs, device="cuda").to(
            torch.int32).reshape(B, S // bs)
        P = torch.full((B,), CTX, device="cuda", dtype=torch.int32)
        L = torch.tensor(lens, device="cuda", dtype=torch.int32)
        # what ragged_step forms once per step, outside the timed glue
        seq = torch.repeat_interleave(torch.arange(B, device="cuda"), L.long())
        starts = torch.cumsum(L.long(), 0) - L
        pos = CTX + torch.arange(T, device="cuda") - starts[seq]
        pos32, src = pos.to(torch.int32), torch.arange(T, device="cuda")

        def glue():
            q, k, v = blocks.prefill_qkv(qkv, pos32, cfg)
            kc[seq, :, pos] = k.index_select(0, src)
            vc[seq, :, pos] = v.index_select(0, src)
            return q

        arms = {"torch_glue": glue,
                "chunk_kernel": lambda: ops.rope_append_kv_chunk_paged(
                    qkv, kp, vp, tables, P, L, max(lens), HQ, HK,
                    cfg.rope_theta)}
        tag = "append_T" + "+".join(str(n) for n in lens)
        for arm, values in alternate(torch, arms).items():
            res[f"{tag}_{arm}_us"] = summary(values, "us")


def engine_mode(torch, ops, res):
    from wva_amd.calibration.model import LLAMA_3_8B, LlamaDecodeModel

    Bp, C = len(CHUNK_LENS), max(CHUNK_LENS)
    kw = dict(max_batch=DECODE_BATCH + Bp, max_seq=CTX + C + 64)
    cont = LlamaDecodeModel(LLAMA_3_8B, **kw)
    paged = LlamaDecodeModel(LLAMA_3_8B, kv_layout="paged", block_size=16, **kw)
    cont.reset(DECODE_BATCH + Bp, CTX)
    paged.reset(DECODE_BATCH + Bp, CTX, headroom=C + 64)
    lens0 = cont.context_lens.clone()
    g = torch.Generator(device="cuda").manual_seed(0)
    dec = torch.randint(0, cont.cfg.vocab_size, (DECODE_BATCH,),
                        device="cuda", generator=g)
    packed = torch.randint(0, cont.cfg.vocab_size, (sum(CHUNK_LENS),),
                           device="cuda", generator=g)
    c_lens = torch.tensor(CHUNK_LENS, dtype=torch.int32, device="cuda")
    arms = {"ragged_step": (cont, cont.ragged_step),
            "paged_ragged_step": (paged, paged.paged_ragged_step)}

    def window(m, step, iters=8):
        """median wall ms of one iteration; context_lens put back first"""
        times = []
        for _ in range(iters):
            m.context_lens.copy_(lens0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(dec, packed, c_lens, C)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1000.0)
        return statistics.median(times)

    for m, step in arms.values():      # warm every shape
        window(m, step, iters=3)
    out = {name: [] for name in arms}
    for _ in range(WINDOWS):
        for name, (m, step) in arms.items():
            out[name].append(window(m, step))
    tag = "x".join(str(n) for n in CHUNK_LENS)
    for name, values in out.items():
        res[f"itl_b{DECODE_BATCH}_ctx{CTX}_chunks{tag}_{name}_ms"] = summary(
            values, "ms")


def worker(mode, out_json):
    sys.path.insert(0, REPO)
    import torch
    from wva_amd import ops

    if not torch.cuda.is_available():
        sys.exit("paged_extend_ab.py measures on a GPU; none found")
    ops._require_ext()
    res = {}
    {"attn": attn_mode, "append": append_mode,
     "engine": engine_mode}[mode](torch, ops, res)
    res["device"] = torch.cuda.get_device_name(0)
    res["arch"] = torch.cuda.get_device_properties(0).gcnArchName
    with open(out_json, "w") as f:
        json.dump(res, f)
    print(f"{mode}: {len(res) - 2} figures", flush=True)


def main(out_json):
    os.makedirs(os.path.dirname(out_json), exist_ok=True)
    merged = {"model": "Llama-3-8B bf16 (random weights)",
              "attention_shape": f"Hq={HQ} Hk={HK} B=1",
              "windows_per_figure": WINDOWS}
    for mode, limit in (("attn", 300), ("append", 120), ("engine", 300)):
        part = f"{out_json}.{mode}.part"
        cmd = ["timeout", "-k", "10", str(limit), sys.executable,
               os.path.abspath(__file__), "worker", mode, part]
        print("+", " ".join(cmd[4:]), flush=True)
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"child {mode} exited {rc}; stopping", flush=True)
            sys.exit(rc if rc > 0 else 1)
        with open(part) as f:
            merged.update(json.load(f))
        os.remove(part)
    with open(out_json, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    for name, r in merged.items():
        if isinstance(r, dict):
            print(f"{name:58s} median {r['median']:10.2f} {r['unit']:3s} "
                  f"spread {r['spread']:8.2f}")
        else:
            print(f"{name:58s} {r}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "worker":
        worker(*sys.argv[2:4])
    else:
        main(os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else
                             os.path.join(REPO, "profiles",
                                          "paged_extend_ab.json")))
