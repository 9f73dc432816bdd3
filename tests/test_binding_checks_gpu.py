"""Argument checks of the raw extension that the older op of each family
(contiguous decode attention, contiguous KV append, prefill) shares with its
newer sibling. Every call must raise before anything is launched.

Every mis-sized operand is a leading-dimension view of a buffer that is large
enough (k[:1] of a 2-sequence cache, lens[:1], a 64-wide view of a buffer four
times the size), so a launch would stay in bounds even if a check were
missing: no test here depends on a kernel misbehaving.
"""
import pytest
import torch

from wva_amd import ops

pytestmark = pytest.mark.gpu

B, HQ, HK, D, S = 2, 8, 2, 128, 192
SCALE = D ** -0.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def caches(dev):
    k = torch.zeros(B, HK, S, D, device=dev, dtype=torch.bfloat16)
    return k, torch.zeros_like(k)


def index(dev, value):
    """(int32 [B], the same values as a strided view of a [2B] buffer)."""
    t = torch.full((B,), value, device=dev, dtype=torch.int32)
    return t, torch.full((2 * B,), value, device=dev, dtype=torch.int32)[::2]


def narrow_cache(dev):
    """A contiguous [B, HK, S, 64] view at the start of a full-size cache."""
    buf = torch.zeros(2 * B, HK, S, D, device=dev, dtype=torch.bfloat16)
    return buf.view(-1)[: B * HK * S * 64].view(B, HK, S, 64)


def test_decode_attn_checks(dev):
    ext = ops._require_ext()
    q = torch.zeros(B, HQ, D, device=dev, dtype=torch.bfloat16)
    (k, v), (lens, strided) = caches(dev), index(dev, 5)
    with pytest.raises(RuntimeError, match="context_lens"):
        ext.gqa_decode_attn(q, k, v, lens[:1], SCALE)
    with pytest.raises(RuntimeError, match="int32"):
        ext.gqa_decode_attn(q, k, v, lens.long(), SCALE)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.gqa_decode_attn(q, k, v, strided, SCALE)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.gqa_decode_attn(q, k, v, lens.cpu(), SCALE)
    with pytest.raises(RuntimeError, match="fewer than B"):
        ext.gqa_decode_attn(q, k[:1], v[:1], lens, SCALE)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ext.gqa_decode_attn(q, k, v[:1], lens, SCALE)
    narrow = narrow_cache(dev)
    with pytest.raises(RuntimeError, match="128"):
        ext.gqa_decode_attn(q, narrow, narrow, lens, SCALE)
    for n in (0, 65536):
        with pytest.raises(RuntimeError, match="num_splits"):
            ext.gqa_decode_attn(q, k, v, lens, SCALE, num_splits=n)


def test_rope_append_kv_checks(dev):
    ext = ops._require_ext()
    qkv = torch.zeros(B, (HQ + 2 * HK) * D, device=dev, dtype=torch.bfloat16)
    (k, v), (pos, strided) = caches(dev), index(dev, 3)
    with pytest.raises(RuntimeError, match="positions"):
        ext.rope_append_kv(qkv, k, v, pos[:1], HQ, HK)
    with pytest.raises(RuntimeError, match="int32"):
        ext.rope_append_kv(qkv, k, v, pos.long(), HQ, HK)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.rope_append_kv(qkv, k, v, strided, HQ, HK)
    with pytest.raises(RuntimeError, match="fewer than B"):
        ext.rope_append_kv(qkv, k[:1], v[:1], pos, HQ, HK)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ext.rope_append_kv(qkv, k, v[:1], pos, HQ, HK)
    q, k2 = (torch.zeros(B, h, D, device=dev, dtype=torch.bfloat16)
             for h in (HQ, HK))
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.rope(q, k2, strided)


def test_prefill_attn_checks(dev):
    ext = ops._require_ext()
    seq = 4
    q = torch.zeros(B * seq, HQ, D, device=dev, dtype=torch.bfloat16)
    k, v = caches(dev)
    with pytest.raises(RuntimeError, match="fewer than B"):
        ext.prefill_attn(q, k[:1], v[:1], B, seq, SCALE)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ext.prefill_attn(q, k, v[:1], B, seq, SCALE)
    narrow = narrow_cache(dev)
    with pytest.raises(RuntimeError, match="128"):
        ext.prefill_attn(q, narrow, narrow, B, seq, SCALE)
