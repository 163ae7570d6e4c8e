"""Opt-in FP8 projection weights (W8A16) on the CPU: the row quantiser's format (e4m3fn bytes [N, K] and
one E8M0 exponent byte per output row: the KV cache's rule along K), the FP8 fragment layout the
streaming decode GEMM reads, the engine option (``LLMEngine(weight_dtype="fp8")``, ``DAB_WEIGHT_DTYPE``,
the ``WEIGHT_DTYPE`` serving setting) and the CPU model, which computes on the dequantised weights."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams
from django_assistant_bot_amd.models import AttnMeta, KVCache, LlamaModel, decoder_config, random_decoder_weights
from django_assistant_bot_amd.ops import reference as ref

PROJ = ("qkv_w", "o_w", "gate_up_w", "down_w")


# ------------------------------------------------------------------------------------------------- layout


@pytest.mark.parametrize("group", [1, 8])
def test_fragment_layout_round_trip_and_index_formula(group):
    """[N/16][K/64][64 lanes][16 B]: lane l holds row l & 15; bytes 0-7 are k = 64j + 8(l >> 4) .. + 8,
    bytes 8-15 k = 64j + 32 + 8(l >> 4) .. + 8.  Grouped: the fragments of G consecutive row blocks
    adjacent per 64-deep k step, fragment (b, j) at ((b // G) K/64 + j) G + b % G KB."""
    N, K = 16 * 8 * 2, 64 * 3
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (N, K), dtype=torch.uint8, generator=g)
    f = ops.shuffle_weights_fp8(data, group)
    assert f.shape == data.shape and f.dtype == torch.uint8 and f.is_contiguous()
    assert torch.equal(ops.unshuffle_weights_fp8(f, group), data)
    assert not torch.equal(f, data)
    flat = f.reshape(-1)
    # one spot per lane quadrant (l >> 4) and k half, in different blocks / k steps / byte positions
    spots = [(b, j, 16 * q + r, 8 * half + i)
             for (b, j, r, i), q, half in zip([(0, 0, 0, 0), (3, 1, 5, 7), (9, 2, 15, 3), (15, 0, 8, 1),
                                               (7, 2, 1, 6), (12, 1, 11, 2), (1, 0, 3, 5), (10, 2, 14, 4)],
                                              [0, 1, 2, 3, 0, 1, 2, 3], [0, 0, 0, 0, 1, 1, 1, 1])]
    assert {(lane >> 4, byte >> 3) for _, _, lane, byte in spots} == {(q, h) for q in range(4) for h in range(2)}
    for b, j, lane, byte in spots:
        frag = ((b // group) * (K // 64) + j) * group + b % group
        n = 16 * b + (lane & 15)
        k = 64 * j + 32 * (byte >> 3) + 8 * (lane >> 4) + (byte & 7)
        assert int(flat[frag * 1024 + lane * 16 + byte]) == int(data[n, k]), (b, j, lane, byte)


def test_fragment_layout_refuses_bad_shapes():
    z = torch.zeros((32, 96), dtype=torch.uint8)
    with pytest.raises(Exception, match="K % 64"):
        ops.shuffle_weights_fp8(z)
    with pytest.raises(Exception, match="16 group"):
        ops.shuffle_weights_fp8(torch.zeros((32, 64), dtype=torch.uint8), 8)
    with pytest.raises(Exception, match="uint8"):
        ops.shuffle_weights_fp8(torch.zeros((32, 64), dtype=torch.bfloat16))


# ---------------------------------------------------------------------------------------------- quantiser


def _rows(seed=1, n_per=8, K=256):
    """bf16 rows with magnitudes 2^-12 .. 2^3 (amax anywhere in its binade)."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for e in range(-12, 4):
        x = torch.randn(n_per, K, generator=g)
        rows.append(x / x.abs().amax(-1, keepdim=True) * 2.0 ** e * (1 + torch.rand(n_per, 1, generator=g)))
    return torch.cat(rows).bfloat16()


def test_quantiser_is_the_kv_row_rule_and_reexported():
    w = _rows()
    data, exps = ops.weight_quantize_fp8(w)
    assert data.dtype == torch.uint8 and data.shape == w.shape and exps.dtype == torch.uint8 and exps.shape == (w.shape[0],)
    kd, ke = ref.kv_quantize(w)
    assert torch.equal(data, kd) and torch.equal(exps, ke)
    dq = ops.weight_dequantize_fp8(data, exps)
    assert dq.dtype == torch.bfloat16 and torch.equal(dq.float(), ref.kv_dequantize(data, exps))  # bf16-exact
    assert ops.weight_quantize_fp8 is ref.weight_quantize_fp8 and ops.weight_dequantize_fp8 is ref.weight_dequantize_fp8


def test_element_error_bound_derived_from_the_format():
    """|w - dq(w)| <= max(2^-4 |w|, 2^-10 s), s = 2^(b - 127): half an ulp of the 3 mantissa bits in the
    normal range, half the 2^-9 spacing of e4m3's lowest binade (and its subnormals) below it."""
    w = _rows(seed=2)
    data, exps = ref.weight_quantize_fp8(w)
    dq = ref.weight_dequantize_fp8(data, exps).float()
    s = torch.exp2(exps.float() - 127)[:, None]
    wf = w.float()
    bound = torch.maximum(wf.abs() * 2.0 ** -4, s * 2.0 ** -10)
    err = (wf - dq).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((err > 0).any())  # (the inputs are not representable: the bound is exercised)
    assert torch.equal(dq.bfloat16().float(), dq)
    assert bool(((wf.abs().amax(-1) / s[:, 0]) <= 448).all()) and bool(((wf.abs().amax(-1) / s[:, 0]) > 224).all())


def test_zero_row_amax_448_and_the_mantissa_boundary():
    K = 64
    w = torch.zeros(5, K, dtype=torch.bfloat16)
    w[1, 3] = 448.0 * 2.0 ** -9  # amax exactly 448 x 2^e: keeps byte value 448
    w[1, 7] = -448.0 * 2.0 ** -9
    w[2, 0] = 1.75 * 2.0 ** -3  # 1.75 x 2^E = 448 x 2^(E - 8): still the smaller exponent
    w[3, 0] = 1.7578125 * 2.0 ** -3  # the next bf16 above 1.75: the larger exponent
    w[4, 0] = 1.0
    data, exps = ref.weight_quantize_fp8(w)
    assert int(exps[0]) == 127 and int(data[0].max()) == 0
    e4 = data.view(torch.float8_e4m3fn).float()
    assert int(exps[1]) == 127 - 9 and float(e4[1, 3]) == 448.0 and float(e4[1, 7]) == -448.0
    assert int(exps[2]) == 127 - 3 - 8 and float(e4[2, 0]) == 448.0
    assert int(exps[3]) == 127 - 3 - 7 and float(e4[3, 0]) == 224.0  # 1.7578 x 128 = 225 -> 224 (spacing 16)
    assert int(exps[4]) == 127 - 8 and float(e4[4, 0]) == 256.0
    dq = ref.weight_dequantize_fp8(data, exps)
    assert torch.equal(dq[:3], w[:3]) and torch.equal(dq[4], w[4])


def test_cpu_stream_gemm_takes_fp8_weights():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(64, 128, generator=g) * 0.05).bfloat16()
    x = torch.randn(5, 128, generator=g).bfloat16()
    data, exps = ops.weight_quantize_fp8(w)
    dq = ops.weight_dequantize_fp8(data, exps)
    assert torch.equal(ops.stream_gemm(x, data, w_exps=exps), ops.stream_gemm(x, dq))
    assert torch.equal(ops.stream_gemm(x, data, w_exps=exps, splits=2), ops.stream_gemm(x, dq, splits=2))


# -------------------------------------------------------------------------------------------------- model


def _weights(cfg=None):
    cfg = cfg or decoder_config("tiny-llama")
    return {k: v.float() for k, v in random_decoder_weights(cfg, dtype=torch.float32, seed=3).items()}


def _dequantised(weights):
    out = dict(weights)
    for k, v in weights.items():
        if k.endswith(PROJ):
            out[k] = ref.weight_dequantize_fp8(*ref.weight_quantize_fp8(v)).to(v.dtype)
    return out


def test_cpu_model_equals_a_default_model_on_the_dequantised_weights():
    cfg = decoder_config("tiny-llama")
    w = _weights(cfg)
    m8 = LlamaModel(cfg, dict(w), "cpu", weight_dtype="fp8")
    m16 = LlamaModel(cfg, _dequantised(w), "cpu")
    assert m8.weight_dtype == "fp8" and m16.weight_dtype == "bf16"
    assert isinstance(m8.layers[0].qkv_w, torch.Tensor) and not torch.equal(m8.layers[0].qkv_w, w["l0.qkv_w"])
    assert torch.equal(m8.embed, m16.embed) and torch.equal(m8.lm_head, m16.lm_head)  # not quantised
    T = 21
    ids = torch.arange(7, 7 + T, dtype=torch.int32)
    outs = []
    for m in (m8, m16):
        kv = KVCache(cfg.layers, 4, cfg.kv_heads, 16, cfg.head_dim, "cpu", dtype=torch.float32)
        meta = AttnMeta(decode=False, positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T),
                        block_tables=torch.arange(4, dtype=torch.int32)[None], ctx_lens=torch.tensor([T], dtype=torch.int32),
                        cu_q=torch.tensor([0, T], dtype=torch.int32), max_q=T)
        h = m.forward(ids, meta, kv)
        outs.append((h, m.logits(h[-1:]), kv.k.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="weight_dtype"):
        LlamaModel(cfg, dict(w), "cpu", weight_dtype="int8")
    with pytest.raises(ValueError, match="tensor parallelism"):
        LlamaModel(cfg, dict(w), "cpu", weight_dtype="fp8", tp_size=2, tp_rank=0)


# ------------------------------------------------------------------------------------------------- engine


def _engine(weights, **kw):
    args = dict(device="cpu", weights=dict(weights), max_batch=8, block_size=16, num_blocks=64, max_prefill_tokens=256,
                use_graphs=False)
    args.update(kw)
    return LLMEngine(decoder_config("tiny-llama"), **args)


def test_engine_option_and_stats():
    w = _weights()
    greedy = SamplingParams(max_new_tokens=8, do_sample=False, temperature=0.0, ignore_eos=True)
    toks = []
    for eng in (_engine(w, weight_dtype="fp8"), _engine(_dequantised(w)), _engine(w, weight_dtype="fp8", kv_cache_dtype="fp8")):
        rids = [eng.add_request(list(range(5, 5 + n)), greedy) for n in (20, 37, 9)]
        while eng.has_unfinished():
            eng.step()
        toks.append([eng.pop_output(r).token_ids for r in rids])
    assert toks[0] == toks[1] and all(len(t) == 8 for t in toks[2])
    e8, e16 = _engine(w, weight_dtype="fp8"), _engine(w)
    assert e8.weight_dtype == "fp8" and e8.model.weight_dtype == "fp8" and e8.stats["weight_bits"] == 8
    assert e16.weight_dtype == "bf16" and e16.model.weight_dtype == "bf16" and e16.stats["weight_bits"] == 16
    assert _engine(w, weight_dtype="bf16").stats["weight_bits"] == 16
    assert isinstance(e8.stats["weight_bits"], int)


def test_engine_refuses_what_is_unsupported():
    w = _weights()
    with pytest.raises(ValueError, match="weight_dtype"):
        _engine(w, weight_dtype="int8")
    with pytest.raises(ValueError, match="weight_dtype.*tensor parallelism"):
        _engine(w, weight_dtype="fp8", tp_size=2)


def test_shared_model_decides_the_dtype():
    w = _weights()
    e8 = _engine(w, weight_dtype="fp8")
    second = _engine(w, shared_model=e8.model)
    assert second.weight_dtype == "fp8" and second.stats["weight_bits"] == 8 and second.model is e8.model
    assert _engine(w, shared_model=e8.model, weight_dtype="fp8").weight_dtype == "fp8"
    with pytest.raises(ValueError, match="weight_dtype"):
        _engine(w, shared_model=e8.model, weight_dtype="bf16")
    e16 = _engine(w)
    with pytest.raises(ValueError, match="weight_dtype"):
        _engine(w, shared_model=e16.model, weight_dtype="fp8")
    assert _engine(w, shared_model=e16.model).weight_dtype == "bf16"


def test_environment_variable_selects_the_weights(monkeypatch):
    w = _weights()
    monkeypatch.setenv("DAB_WEIGHT_DTYPE", "fp8")
    assert _engine(w).weight_dtype == "fp8"
    assert _engine(w, weight_dtype="bf16").weight_dtype == "bf16"  # the argument wins
    monkeypatch.setenv("DAB_WEIGHT_DTYPE", "fp4")
    with pytest.raises(ValueError, match="weight_dtype"):
        _engine(w)
    monkeypatch.delenv("DAB_WEIGHT_DTYPE")
    assert _engine(w).weight_dtype == "bf16"


def test_serving_setting_reaches_the_engine(monkeypatch):
    from django_assistant_bot_amd.engine import llm_engine, serving

    seen = {}

    class _Eng:
        def __init__(self, model, **kw):
            seen.update(kw)

    monkeypatch.setattr(llm_engine, "LLMEngine", _Eng)  # (get_llm_worker imports it when called)
    monkeypatch.setattr(serving, "LLMWorker", lambda e: e)
    monkeypatch.setattr(serving, "setting", lambda name, default: "fp8" if name == "WEIGHT_DTYPE" else default)
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["weight_dtype"] == "fp8" and seen["kv_cache_dtype"] is None
    seen.clear()
    monkeypatch.setattr(serving, "setting", lambda name, default: default)
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["weight_dtype"] is None  # the engine then reads the environment, else bf16
