"""The opt-in FP8 KV cache on the CPU oracle: the quantiser's format (one E8M0 exponent byte and 128
e4m3fn bytes per (token, kv head) row), the FP8 forms of the three cache ops on the needle cases of
tests/attn_cases.py, and the engine option (``LLMEngine(kv_cache_dtype="fp8")``, ``DAB_KV_CACHE_DTYPE``)."""
import math

import pytest
import torch

import attn_cases as ac
import kv_fp8_cases as fc
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams
from django_assistant_bot_amd.models import AttnMeta, KVCache, LlamaModel, decoder_config, random_decoder_weights
from django_assistant_bot_amd.models.configs import DecoderConfig
from django_assistant_bot_amd.ops import reference as ref

E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
E4M3 = E4M3[torch.isfinite(E4M3)]  # every representable value (both zeros)


# ---------------------------------------------------------------------------------------------- quantiser


def test_representable_values_round_trip_bit_exact():
    """Rows of representable values times a power of two whose amax fills the top binade of the format
    (256 .. 448 before scaling) come back bit for bit, and re-quantise to the same bytes."""
    g = torch.Generator().manual_seed(0)
    for k in (-30, -7, 0, 3, 20):
        x = E4M3[torch.randint(0, E4M3.numel(), (64, 128), generator=g)]
        x[:, 0] = 448.0 - 32.0 * torch.arange(64).remainder(7)  # amax in [256, 448]: exponent exactly k
        x = (x * 2.0 ** k).bfloat16()
        assert torch.equal(x.float(), x.float().bfloat16().float())
        data, b = ref.kv_quantize(x)
        assert data.dtype == torch.uint8 and b.dtype == torch.uint8 and data.shape == x.shape and b.shape == x.shape[:-1]
        assert torch.equal(b, torch.full_like(b, 127 + k))
        deq = ref.kv_dequantize(data, b)
        assert torch.equal(deq, x.float())
        d2, b2 = ref.kv_quantize(deq.bfloat16())
        assert torch.equal(d2, data) and torch.equal(b2, b)


def test_error_bound_and_bf16_exactness_over_the_range():
    """|deq - x| <= amax / 16 per row, and every dequantised value is a bf16, for amax 2^-20 .. 2^10."""
    g = torch.Generator().manual_seed(1)
    worst = 0.0
    for e in range(-20, 11):
        x = torch.randn(256, 128, generator=g)
        x = (x / x.abs().amax(-1, keepdim=True) * 2.0 ** e * (1 + torch.rand(256, 1, generator=g))).bfloat16()
        data, b = ref.kv_quantize(x)
        deq = ref.kv_dequantize(data, b)
        amax = x.float().abs().amax(-1, keepdim=True)
        assert bool(((deq - x.float()).abs() <= amax / 16).all()), e
        assert torch.equal(deq.bfloat16().float(), deq)
        worst = max(worst, float(((deq - x.float()).abs() / amax).max()))
    print(f"largest |deq - x| / amax = {worst:.4f} (1/{1 / worst:.1f})")


def test_zero_row():
    x = torch.zeros(3, 128, dtype=torch.bfloat16)
    x[1, 5] = -0.0
    data, b = ref.kv_quantize(x)
    assert torch.equal(b, torch.full((3,), 127, dtype=torch.uint8)) and int(data.max()) == 0
    assert torch.equal(ref.kv_dequantize(data, b), torch.zeros(3, 128))


def test_exponent_rule_at_the_edges():
    """amax = 448 x 2^k still takes exponent k (its byte is 0x7e = 448); the next bf16 above it (450 x 2^k,
    mantissa 0x61 > 0x60) takes k + 1.  The rule is the frexp one of the format's definition."""
    for k in (-40, -9, -1, 0, 1, 17, 60):
        top = torch.tensor(448.0 * 2.0 ** k).bfloat16()
        nxt = (top.view(torch.int16) + 1).view(torch.bfloat16)
        assert float(nxt) > float(top) and float(nxt) == 450.0 * 2.0 ** k
        x = torch.zeros(2, 128, dtype=torch.bfloat16)
        x[0, 7], x[1, 100] = top, -nxt
        x[:, 0] = 2.0 ** k  # a small companion
        data, b = ref.kv_quantize(x)
        assert b.tolist() == [127 + k, 128 + k]
        assert int(data[0, 7]) == 0x7E and int(data[1, 100]) == 0xF6  # 448 ; -(450 / 2 -> 224 = 1.75 x 2^7)
        for row in x.float():
            m, e = math.frexp(float(row.abs().max()))
            want = e - 9 if m <= 0.875 else e - 8
            bb = int(ref.kv_quantize(row.bfloat16()[None])[1])
            assert bb == want + 127
            assert float(row.abs().max()) / 2.0 ** want <= 448 < float(row.abs().max()) / 2.0 ** (want - 1)


def test_exponent_byte_is_clamped():
    x = torch.zeros(2, 128, dtype=torch.bfloat16)
    x[0, 0] = 2.0 ** -125  # e + 127 would be -6
    x[1, 0] = 2.0 ** 127
    data, b = ref.kv_quantize(x)
    assert b.tolist() == [1, 246]
    assert torch.equal(ref.kv_dequantize(data, b), x.float())


# ---------------------------------------------------------------------------------------------- the three ops


DECODE = ["dec_a-s8", "dec_b-p512", "dec_d-bs32-s0", "dec_e-g16-s0"]
PREFILL = ["pre_f-c", "pre_g", "pre_long"]


def _assert(view, out, tag):
    rep = ac.check(view, out)
    print(f"KVFP8 oracle case={tag} err/f={rep.ratio} f={rep.f} tau={rep.tau} needle_dev={rep.needle_dev}")
    assert rep.ok, str(rep)
    assert rep.tau is None or rep.tau <= ac.TAU_CAP
    return rep


@pytest.mark.parametrize("name", DECODE + PREFILL)
def test_needle_cases_through_the_fp8_oracle(name):
    """Position codes and needle keys quantise exactly: every needle row still returns its code; the
    plain forms pass the relative check against the fp64 reference of the dequantised values."""
    for needles in (True, False):
        view, cache = fc.get_fp8(name, "cpu", needles)
        if needles:
            base = ac.get_case(name, "cpu", True)
            assert torch.equal(view.v, base.v)  # the codes are representable
            rep = _assert(view, fc.run_fp8(view, cache, ops), f"{name}/needles")
            assert rep.needle_dev == 0.0
        else:
            _assert(view, fc.run_fp8(view, cache, ops), f"{name}/plain")


def test_row_scaled_case_sees_a_wrong_exponent():
    """The row-scaled plain form passes, and fails once the exponent bytes are shifted by one slot."""
    view, cache = fc.get_fp8("dec_d-bs32-s0", "cpu", False, True)
    _assert(view, fc.run_fp8(view, cache, ops), "dec_d-bs32-s0/scaled")
    kd, ke, vd, ve = cache
    for broken in ((kd, ke.roll(1, -1), vd, ve), (kd, ke, vd, ve.roll(1, -1))):
        assert not ac.check(view, fc.run_fp8(view, broken, ops)).ok


def test_writer_oracle_quantises_what_the_bf16_cache_holds():
    T, Hq, Hkv, D, bs = 19, 4, 2, 128, 16
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, generator=g).bfloat16()
    qkv[5] = 0
    pos = torch.arange(T, dtype=torch.int32)
    cs = ref.rope_cos_sin(ref.llama3_inv_freq(D, 10000.0, None), 64)
    slots = torch.randperm(3 * bs, generator=g)[:T]
    slots[3] = -1
    kb = torch.zeros(3, Hkv, bs, D, dtype=torch.bfloat16)
    vb = torch.zeros_like(kb)
    q0 = ops.rope_kv_write(qkv, pos, cs, kb, vb, slots, Hq, Hkv, D)
    cache = [torch.full((3, Hkv, bs, D), 0x55, dtype=torch.uint8), torch.full((3, Hkv, bs), 0x55, dtype=torch.uint8),
             torch.full((3, Hkv, bs, D), 0x55, dtype=torch.uint8), torch.full((3, Hkv, bs), 0x55, dtype=torch.uint8)]
    q1 = ops.rope_kv_write_fp8(qkv, pos, cs, *cache, slots, Hq, Hkv, D)
    assert torch.equal(q0, q1)
    written = torch.zeros(3 * bs, dtype=torch.bool)
    written[slots[slots >= 0]] = True
    w = written.view(3, 1, bs).expand(3, Hkv, bs)
    for (data, exps), bf in ((cache[:2], kb), (cache[2:], vb)):
        d, e = ref.kv_quantize(bf)
        assert torch.equal(data[w], d[w]) and torch.equal(exps[w], e[w])
        assert bool((data[~w] == 0x55).all()) and bool((exps[~w] == 0x55).all())
    assert ops.rope_kv_write_fp8(qkv, pos, cs, *cache, slots, Hq, Hkv, D, write_q=False) is None


def test_dequant_blocks_oracle_and_plan():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 2, 16, 128, generator=g).bfloat16()
    kd, ke = ref.kv_quantize(x)
    vd, ve = ref.kv_quantize((x * 3).bfloat16())
    ids = torch.tensor([4, 1, 5], dtype=torch.int32)
    ko = torch.full((5, 2, 16, 128), 9.0, dtype=torch.bfloat16)
    vo = torch.full_like(ko, 9.0)
    ops.kv_dequant_blocks(kd, ke, vd, ve, ids, ko, vo)
    assert torch.equal(ko[:3].float(), ref.kv_dequantize(kd, ke)[ids.long()])
    assert torch.equal(vo[:3].float(), ref.kv_dequantize(vd, ve)[ids.long()])
    assert bool((ko[3:] == 9).all()) and bool((vo[3:] == 9).all())
    # plan: 4 sequences of 3 / 1 / 2 / 2 blocks into a scratch of 4 -> groups {0, 1}, {2, 3}
    bt = torch.tensor([[7, 8, 9, 0], [3, 0, 0, 0], [5, 6, 0, 0], [1, 2, 0, 0]], dtype=torch.int32)
    plan = ops.kv_prefill_plan(bt, [40, 16, 17, 32], [0, 40, 41, 58, 60], 16, 4)
    assert plan.blocks.tolist() == [7, 8, 9, 3, 5, 6, 1, 2]
    assert [g[:7] for g in plan.groups] == [(0, 2, 0, 4, 0, 41, 40), (2, 4, 4, 8, 41, 60, 17)]
    assert [g[7].tolist() for g in plan.groups] == [[0, 40, 41], [0, 17, 19]]
    assert plan.scratch_bt.tolist() == [[0, 1, 2, 0], [3, 3, 3, 3], [0, 1, 0, 0], [2, 3, 2, 2]]
    one = ops.kv_prefill_plan(bt, [40, 16, 17, 32], [0, 40, 41, 58, 60], 16, 8)
    assert len(one.groups) == 1 and one.groups[0][7] is None
    with pytest.raises(ValueError, match="exceeds the FP8 prefill scratch"):
        ops.kv_prefill_plan(bt, [40, 16, 17, 32], [0, 40, 41, 58, 60], 16, 2)


def test_warm_is_refused():
    view, cache = fc.get_fp8("dec_e-g2-s0", "cpu", True)
    with pytest.raises(ValueError, match="warm"):
        fc.run_fp8(view, cache, ops, warm=([(view.q, 16)], 4))


# ---------------------------------------------------------------------------------------------- model and engine

TOY = DecoderConfig("toy-d128", vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, intermediate=1024,
                    max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)


def _prefill(model, cfg, ids, bs=64, nb=8):
    kv = KVCache(cfg.layers, nb, cfg.kv_heads, bs, cfg.head_dim, "cpu", dtype=torch.float32, kv_dtype="fp8")
    T = len(ids)
    meta = AttnMeta(decode=False, positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T),
                    block_tables=torch.arange(nb, dtype=torch.int32)[None], ctx_lens=torch.tensor([T], dtype=torch.int32),
                    cu_q=torch.tensor([0, T], dtype=torch.int32), max_q=T)
    return model.forward(torch.tensor(ids, dtype=torch.int32), meta, kv), kv


@pytest.mark.parametrize("cfg", [decoder_config("tiny-llama"), TOY], ids=["d64", "d128"])
def test_llama_decode_consistent_with_prefill_fp8(cfg):
    """test_llama_decode_consistent_with_prefill on an FP8 cache, at that test's bound: the decode step
    and the prefill read the same dequantised K / V."""
    full = {k: v.float() for k, v in random_decoder_weights(cfg, dtype=torch.float32, seed=2).items()}
    model = LlamaModel(cfg, full, "cpu")
    ids = list(range(3, 3 + 70))  # crosses a 64-token block
    h_full, kv_full = _prefill(model, cfg, ids)
    h_pre, kv = _prefill(model, cfg, ids[:-1])
    assert kv.k.dtype == torch.uint8 and kv.k_exp.shape == (cfg.layers, 8, cfg.kv_heads, 64) and int(kv.k[0, 0].max()) > 0
    T = len(ids)
    meta = AttnMeta(decode=True, positions=torch.tensor([T - 1], dtype=torch.int32), slots=torch.tensor([T - 1]),
                    block_tables=torch.arange(8, dtype=torch.int32)[None], ctx_lens=torch.tensor([T], dtype=torch.int32))
    h_dec = model.forward(torch.tensor([ids[-1]], dtype=torch.int32), meta, kv)
    assert torch.allclose(h_dec[0], h_full[-1], atol=1e-4)
    assert torch.equal(kv.k, kv_full.k) and torch.equal(kv.v_exp, kv_full.v_exp)


def _weights(cfg=None):
    cfg = cfg or decoder_config("tiny-llama")
    return {k: v.float() for k, v in random_decoder_weights(cfg, dtype=torch.float32, seed=3).items()}


def _engine(weights, **kw):
    args = dict(device="cpu", weights=dict(weights), max_batch=8, block_size=16, num_blocks=64, max_prefill_tokens=256,
                use_graphs=False)
    args.update(kw)
    return LLMEngine(decoder_config("tiny-llama"), **args)


def test_engine_generates_with_an_fp8_cache_and_mixed_steps_agree():
    w = _weights()
    greedy = SamplingParams(max_new_tokens=10, do_sample=False, temperature=0.0, ignore_eos=True)
    outs = []
    for mixed in (0, 32):
        eng = _engine(w, kv_cache_dtype="fp8", mixed_prefill_tokens=mixed)
        assert eng.kv_cache_dtype == "fp8" and eng.kv.fp8 and eng.stats["kv_cache_bits"] == 8
        rids = [eng.add_request(list(range(5, 5 + n)), greedy) for n in (20, 37)]
        for _ in range(3):
            eng.step()
        rids += [eng.add_request(list(range(300, 300 + n)), greedy) for n in (50, 9, 70)]
        while eng.has_unfinished():
            eng.step()
        outs.append([eng.pop_output(r).token_ids for r in rids])
        assert (eng.stats["mixed_steps"] > 0) == bool(mixed)
    assert outs[0] == outs[1] and all(len(t) == 10 for t in outs[0])
    assert _engine(w).kv_cache_dtype == "bf16" and _engine(w).stats["kv_cache_bits"] == 16


def test_block_count_follows_the_fp8_block_size():
    cfg = decoder_config("tiny-llama")
    w = _weights()
    L, H, bs, D = cfg.layers, cfg.kv_heads, 16, cfg.head_dim
    assert KVCache.bytes_per_block(L, H, bs, D, kv_dtype="fp8") == 2 * L * H * bs * (D + 1)
    assert KVCache.bytes_per_block(L, H, bs, D) == 2 * L * H * bs * D * 2
    gb = 100 * 2 * L * H * bs * (D + 1) / (1 << 30)  # room for exactly 100 FP8 blocks
    n8 = _engine(w, num_blocks=None, kv_cache_gb=gb, kv_cache_dtype="fp8", max_model_len=512).kv.num_blocks
    n16 = _engine(w, num_blocks=None, kv_cache_gb=gb, max_model_len=512).kv.num_blocks
    assert n8 == 100 and n16 == int(100 * (D + 1) / (2 * D))


def test_engine_refuses_what_is_unsupported():
    w = _weights()
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        _engine(w, kv_cache_dtype="int8")
    with pytest.raises(ValueError, match="tensor parallelism"):
        _engine(w, kv_cache_dtype="fp8", tp_size=2)
    with pytest.raises(ValueError, match="head_dim 128"):  # raised before anything touches the device
        _engine(w, kv_cache_dtype="fp8", device="cuda")
    with pytest.raises(ValueError):
        KVCache(1, 2, 1, 16, 64, "cpu", kv_dtype="e5m2")


def test_environment_variable_selects_the_cache(monkeypatch):
    w = _weights()
    monkeypatch.setenv("DAB_KV_CACHE_DTYPE", "fp8")
    assert _engine(w).kv_cache_dtype == "fp8"
    assert _engine(w, kv_cache_dtype="bf16").kv_cache_dtype == "bf16"  # the argument wins
    monkeypatch.setenv("DAB_KV_CACHE_DTYPE", "fp4")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        _engine(w)
    monkeypatch.delenv("DAB_KV_CACHE_DTYPE")
    assert _engine(w).kv_cache_dtype == "bf16"


def test_serving_setting_reaches_the_engine(monkeypatch):
    from django_assistant_bot_amd.engine import llm_engine, serving

    seen = {}

    class _Eng:
        def __init__(self, model, **kw):
            seen.update(kw)

    monkeypatch.setattr(llm_engine, "LLMEngine", _Eng)  # (get_llm_worker imports it when called)
    monkeypatch.setattr(serving, "LLMWorker", lambda e: e)
    monkeypatch.setattr(serving, "setting", lambda name, default: "fp8" if name == "KV_CACHE_DTYPE" else default)
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["kv_cache_dtype"] == "fp8"
