"""Opt-in MXFP4 projection weights (W4A16) on the CPU: the block quantiser's format (e2m1 codes, two per
byte, and one E8M0 scale byte per 32 k of a row), the MXFP4 fragment layout and the scale layout the
streaming decode GEMM reads, the engine option (``LLMEngine(weight_dtype="mxfp4")``, ``DAB_WEIGHT_DTYPE``,
the ``WEIGHT_DTYPE`` serving setting) and the CPU model, which computes on the dequantised weights."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams
from django_assistant_bot_amd.models import AttnMeta, KVCache, LlamaModel, decoder_config, random_decoder_weights
from django_assistant_bot_amd.ops import reference as ref

PROJ = ("qkv_w", "o_w", "gate_up_w", "down_w")
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _nibbles(codes):
    """uint8 [N, K/2] -> int codes [N, K] in k order (low nibble first)."""
    c = codes.to(torch.int32)
    return torch.stack([c & 15, c >> 4], -1).reshape(codes.shape[0], -1)


def _no_negative_zero(codes):
    return not bool((_nibbles(codes) == 8).any())


# ---------------------------------------------------------------------------------------------- quantiser


def test_scale_rule_at_the_mantissa_boundary_and_reexported():
    """amax = 1.5 x 2^e keeps the lower scale (6 x 2^(e-2) = amax: nothing clips), one ulp above takes the
    next one; b = E - 2 or E - 1 from the bits of amax."""
    rows, want_b = [], []
    for e in (-20, -3, 0, 2, 9):
        lo = torch.tensor(1.5 * 2.0 ** e)
        for amax, b in ((lo, e + 125), (torch.nextafter(lo, torch.tensor(float("inf"))), e + 126),
                        (torch.tensor(1.5078125 * 2.0 ** e), e + 126),  # the next bf16
                        (torch.tensor(1.0 * 2.0 ** e), e + 125), (torch.tensor(1.9921875 * 2.0 ** e), e + 126)):
            r = torch.zeros(32)
            r[5] = -amax
            r[9] = amax / 4
            rows.append(r)
            want_b.append(b)
    w = torch.stack(rows)
    codes, scales = ops.weight_quantize_mxfp4(w)
    assert codes.dtype == torch.uint8 and codes.shape == (len(rows), 16)
    assert scales.dtype == torch.uint8 and scales.shape == (len(rows), 1)
    assert scales[:, 0].tolist() == want_b
    s = torch.exp2(scales.float() - 127)[:, 0]
    ratio = w.abs().amax(-1) / s
    assert bool((ratio <= 6).all()) and bool((ratio > 3).all())  # the SMALLEST power of two that does not clip
    assert _no_negative_zero(codes)
    assert ops.weight_quantize_mxfp4 is ref.weight_quantize_mxfp4
    assert ops.weight_dequantize_mxfp4 is ref.weight_dequantize_mxfp4


def test_tie_midpoints_round_to_the_even_code_in_both_signs():
    mids = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    for scale in (1.0, 2.0 ** -7, 2.0 ** 5):
        r = torch.zeros(2, 32)
        r[0, 0], r[1, 0] = 6.0, -6.0  # amax 6: scale byte 127, the values are their own grid coordinates
        r[0, 1:8] = torch.tensor(mids)
        r[1, 1:8] = -torch.tensor(mids)
        r[0, 8:15] = -torch.tensor(mids)
        codes, scales = ref.weight_quantize_mxfp4(r * scale)
        dq = ref.weight_dequantize_mxfp4(codes, scales).float() / scale
        assert dq[0, 1:8].tolist() == want and dq[1, 1:8].tolist() == [-v for v in want]
        assert dq[0, 8:15].tolist() == [-v for v in want]
        assert dq[0, 0] == 6.0 and dq[1, 0] == -6.0
        n = _nibbles(codes)
        assert n[0, 1:8].tolist() == [0, 2, 2, 4, 4, 6, 6] and n[1, 1:8].tolist() == [0, 10, 10, 12, 12, 14, 14]
        assert _no_negative_zero(codes)  # -0.25 -> code 0, not 8


def test_zero_block_and_both_clamps():
    w = torch.zeros(6, 64)
    w[1, 32 + 3] = 2.0 ** -126   # E = 1: b would be -1 -> 2; 2^-126 = 0.5 x 2^-125 stays exact
    w[1, 32 + 4] = -(2.0 ** -127)  # 0.25 x 2^-125: the tie to zero, stored as +0
    w[2, 0] = 1.5 * 2.0 ** -123  # b = 2 without the clamp: 6 x 2^-125
    w[3, 7] = 1.5 * 2.0 ** 127   # b = 252 without the clamp: 6 x 2^125
    w[4, 7] = -1.75 * 2.0 ** 127  # b would be 253 -> 252: the one value that clips, to -6 x 2^125
    w[4, 8] = 2.0 ** 125
    w[5, 40] = 1.0
    codes, scales = ref.weight_quantize_mxfp4(w)
    assert scales.tolist() == [[127, 127], [127, 2], [2, 127], [252, 127], [252, 127], [127, 125]]
    assert not bool(codes[0].any()) and not bool(codes[1, :16].any())
    dq = ref.weight_dequantize_mxfp4(codes, scales)
    assert dq.dtype == torch.bfloat16
    keep = [0, 2, 3, 5]
    assert torch.equal(dq[keep].float(), w[keep])
    assert float(dq[1, 35]) == 2.0 ** -126 and float(dq[1, 36]) == 0.0
    assert float(dq[4, 7]) == -6.0 * 2.0 ** 125 and float(dq[4, 8]) == 2.0 ** 125
    assert bool(torch.isfinite(dq.float()).all()) and _no_negative_zero(codes)
    with pytest.raises(ValueError, match="K % 32"):
        ref.weight_quantize_mxfp4(torch.zeros(4, 48))


def test_grid_values_round_trip_and_the_error_bound_elsewhere():
    """Blocks already on their grid come back exactly (codes and scale bytes too); anything else lands
    within half the local grid step: 0.25 below 2, 0.5 in [2, 4), 1 in [4, 6] times the scale."""
    g = torch.Generator().manual_seed(0)
    N, K = 64, 256
    n = torch.randint(0, 16, (N, K), generator=g)
    n[n == 8] = 0  # (-0 is never produced)
    n.view(N, K // 32, 32)[:, :, 0] = torch.randint(0, 2, (N, K // 32), generator=g) * 8 + 6 + \
        torch.randint(0, 2, (N, K // 32), generator=g)  # +-4 or +-6 in every block: the scale is determined
    n.view(N, K // 32, 32)[0, 0, :] = torch.tensor([7, 15] * 16)  # (+-6 only)
    codes = (n[:, 0::2] | (n[:, 1::2] << 4)).to(torch.uint8)
    scales = torch.randint(2, 253, (N, K // 32), generator=g).to(torch.uint8)
    scales[0, :4] = torch.tensor([2, 3, 251, 252], dtype=torch.uint8)
    x = ref.weight_dequantize_mxfp4(codes, scales)
    assert x.dtype == torch.bfloat16 and bool(torch.isfinite(x.float()).all())
    lut = torch.tensor(GRID + tuple(-v for v in GRID))
    assert torch.equal(x.float(), (lut[n].view(N, K // 32, 32)
                                   * torch.exp2(scales.double() - 127)[..., None]).reshape(N, K).float())
    c2, s2 = ref.weight_quantize_mxfp4(x)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    assert torch.equal(ref.weight_dequantize_mxfp4(c2, s2), x)
    # off the grid: block magnitudes 2^-12 .. 2^3, amax anywhere in its binade
    w = (torch.randn(N, K, generator=g).view(N, K // 32, 32)
         * torch.exp2(torch.randint(-12, 4, (N, K // 32, 1), generator=g).float())
         * (1 + torch.rand(N, K // 32, 1, generator=g))).reshape(N, K).bfloat16()
    codes, scales = ref.weight_quantize_mxfp4(w)
    dq = ref.weight_dequantize_mxfp4(codes, scales).double().view(N, K // 32, 32)
    s = torch.exp2(scales.double() - 127)[..., None]
    y = (w.double().view(N, K // 32, 32) / s).abs()
    assert bool((y.amax(-1) <= 6).all()) and bool((y.amax(-1) > 3).all())
    half_step = torch.where(y < 2, 0.25, torch.where(y < 4, 0.5, 1.0))
    err = (w.double().view(N, K // 32, 32) - dq).abs()
    assert bool((err <= s * half_step).all()), float((err / (s * half_step)).max())
    assert bool((err > 0).any()) and _no_negative_zero(codes)


# ------------------------------------------------------------------------------------------------- layout


@pytest.mark.parametrize("group", [1, 8])
def test_fragment_layout_round_trip_and_index_formula(group):
    """[N/16][K/128][64 lanes][16 B]: lane l holds row l & 15, its bytes 4c .. 4c + 3 the 8 codes of
    k = 128j + 32c + 8(l >> 4) .. + 8, the lower k of a byte in the low nibble.  Grouped: fragment (b, j) at
    ((b // G) K/128 + j) G + b % G KB.  Scales: [N/16][K/128][16 rows][4 B], whatever the group."""
    N, K = 16 * 8 * 2, 128 * 3
    g = torch.Generator().manual_seed(0)
    n = torch.randint(0, 16, (N, K), generator=g)
    codes = (n[:, 0::2] | (n[:, 1::2] << 4)).to(torch.uint8)
    scales = torch.randint(0, 256, (N, K // 32), dtype=torch.uint8, generator=g)
    f = ops.shuffle_weights_mxfp4(codes, group)
    assert f.shape == codes.shape and f.dtype == torch.uint8 and f.is_contiguous()
    assert torch.equal(ops.unshuffle_weights_mxfp4(f, group), codes) and not torch.equal(f, codes)
    fs = ops.shuffle_scales_mxfp4(scales)
    assert fs.shape == scales.shape and fs.dtype == torch.uint8 and fs.is_contiguous()
    assert torch.equal(ops.unshuffle_scales_mxfp4(fs), scales) and not torch.equal(fs, scales)
    flat, sflat = f.reshape(-1), fs.reshape(-1)
    seen = set()
    # every (chunk, lane quadrant) once, in different rows / blocks / k steps / byte positions, + the corners
    spots = [((37 * i + 5) % N, 128 * (i % 3) + 32 * (i // 4) + 8 * (i % 4) + (3 * i) % 8) for i in range(16)]
    for row, k in spots + [(0, 0), (0, 1), (N - 1, K - 1), (N - 1, K - 2)]:
        b, j, c, q = row // 16, k // 128, (k % 128) // 32, (k % 32) // 8
        lane = 16 * q + row % 16
        frag = ((b // group) * (K // 128) + j) * group + b % group
        byte = int(flat[frag * 1024 + lane * 16 + 4 * c + (k % 8) // 2])
        assert (byte >> 4 if k & 1 else byte & 15) == int(n[row, k]), (row, k)
        assert int(sflat[(b * (K // 128) + j) * 64 + (row % 16) * 4 + c]) == int(scales[row, k // 32]), (row, k)
        seen.add((c, q, k & 1))
    assert {(c, q) for c, q, _ in seen} == {(c, q) for c in range(4) for q in range(4)} and {p for *_, p in seen} == {0, 1}


def test_fragment_layout_refuses_bad_shapes():
    with pytest.raises(Exception, match="K % 128"):
        ops.shuffle_weights_mxfp4(torch.zeros((32, 32), dtype=torch.uint8))  # K = 64
    with pytest.raises(Exception, match="16 group"):
        ops.shuffle_weights_mxfp4(torch.zeros((32, 64), dtype=torch.uint8), 8)
    with pytest.raises(Exception, match="uint8"):
        ops.shuffle_weights_mxfp4(torch.zeros((32, 64), dtype=torch.bfloat16))
    with pytest.raises(Exception, match="K % 128"):
        ops.shuffle_scales_mxfp4(torch.zeros((32, 6), dtype=torch.uint8))


def test_cpu_stream_gemm_takes_mxfp4_weights():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(64, 128, generator=g) * 0.05).bfloat16()
    x = torch.randn(5, 128, generator=g).bfloat16()
    codes, scales = ops.weight_quantize_mxfp4(w)
    dq = ops.weight_dequantize_mxfp4(codes, scales)
    assert not torch.equal(dq, w)
    assert torch.equal(ops.stream_gemm(x, codes, w_scales=scales), ops.stream_gemm(x, dq))
    assert torch.equal(ops.stream_gemm(x, codes, w_scales=scales, splits=2), ops.stream_gemm(x, dq, splits=2))
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.stream_gemm(x, codes, w_scales=scales, w_exps=torch.full((64,), 127, dtype=torch.uint8))


# -------------------------------------------------------------------------------------------------- model


def _weights(cfg=None):
    cfg = cfg or decoder_config("tiny-llama")
    return {k: v.float() for k, v in random_decoder_weights(cfg, dtype=torch.float32, seed=3).items()}


def _dequantised(weights):
    out = dict(weights)
    for k, v in weights.items():
        if k.endswith(PROJ):
            out[k] = ref.weight_dequantize_mxfp4(*ref.weight_quantize_mxfp4(v)).to(v.dtype)
    return out


def test_cpu_model_equals_a_default_model_on_the_dequantised_weights():
    cfg = decoder_config("tiny-llama")
    w = _weights(cfg)
    m4 = LlamaModel(cfg, dict(w), "cpu", weight_dtype="mxfp4")
    m16 = LlamaModel(cfg, _dequantised(w), "cpu")
    assert m4.weight_dtype == "mxfp4" and m16.weight_dtype == "bf16"
    assert isinstance(m4.layers[0].qkv_w, torch.Tensor) and not torch.equal(m4.layers[0].qkv_w, w["l0.qkv_w"])
    assert torch.equal(m4.layers[1].down_w, m16.layers[1].down_w)
    assert torch.equal(m4.embed, m16.embed) and torch.equal(m4.lm_head, m16.lm_head)  # not quantised
    T = 21
    ids = torch.arange(7, 7 + T, dtype=torch.int32)
    outs = []
    for m in (m4, m16):
        kv = KVCache(cfg.layers, 4, cfg.kv_heads, 16, cfg.head_dim, "cpu", dtype=torch.float32)
        meta = AttnMeta(decode=False, positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T),
                        block_tables=torch.arange(4, dtype=torch.int32)[None], ctx_lens=torch.tensor([T], dtype=torch.int32),
                        cu_q=torch.tensor([0, T], dtype=torch.int32), max_q=T)
        h = m.forward(ids, meta, kv)
        outs.append((h, m.logits(h[-1:]), kv.k.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="tensor parallelism"):
        LlamaModel(cfg, dict(w), "cpu", weight_dtype="mxfp4", tp_size=2, tp_rank=0)
    with pytest.raises(ValueError, match="fp8_weights_only"):
        LlamaModel(cfg, dict(w), "cpu", weight_dtype="mxfp4", fp8_weights_only=True)
    with pytest.raises(ValueError, match="weight_dtype"):
        LlamaModel(cfg, dict(w), "cpu", weight_dtype="fp4")


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
    for eng in (_engine(w, weight_dtype="mxfp4"), _engine(_dequantised(w)),
                _engine(w, weight_dtype="mxfp4", kv_cache_dtype="fp8")):
        rids = [eng.add_request(list(range(5, 5 + n)), greedy) for n in (20, 37, 9)]
        while eng.has_unfinished():
            eng.step()
        toks.append([eng.pop_output(r).token_ids for r in rids])
    assert toks[0] == toks[1] and all(len(t) == 8 for t in toks[2])
    e4, e16 = _engine(w, weight_dtype="mxfp4"), _engine(w)
    assert e4.weight_dtype == "mxfp4" and e4.model.weight_dtype == "mxfp4" and e4.stats["weight_bits"] == 4
    assert isinstance(e4.stats["weight_bits"], int) and e16.stats["weight_bits"] == 16
    # the resident tensors, counted: on the CPU the dequantised weights alone
    assert e4.stats["weight_bytes"] == e16.stats["weight_bytes"] == e4.model.projection_bytes() > 0
    assert e4.stats["weight_bf16_copy"] is True


def test_engine_refuses_what_is_unsupported():
    w = _weights()
    with pytest.raises(ValueError, match="weight_dtype.*tensor parallelism"):
        _engine(w, weight_dtype="mxfp4", tp_size=2)
    with pytest.raises(ValueError, match="fp8_weights_only"):
        _engine(w, weight_dtype="mxfp4", fp8_weights_only=True)


def test_shared_model_decides_the_dtype():
    w = _weights()
    e4 = _engine(w, weight_dtype="mxfp4")
    second = _engine(w, shared_model=e4.model)
    assert second.weight_dtype == "mxfp4" and second.stats["weight_bits"] == 4 and second.model is e4.model
    assert _engine(w, shared_model=e4.model, weight_dtype="mxfp4").weight_dtype == "mxfp4"
    for other in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="weight_dtype"):
            _engine(w, shared_model=e4.model, weight_dtype=other)
    for model in (_engine(w).model, _engine(w, weight_dtype="fp8").model):
        with pytest.raises(ValueError, match="weight_dtype"):
            _engine(w, shared_model=model, weight_dtype="mxfp4")


def test_environment_variable_selects_the_weights(monkeypatch):
    w = _weights()
    monkeypatch.setenv("DAB_WEIGHT_DTYPE", "mxfp4")
    assert _engine(w).weight_dtype == "mxfp4"
    assert _engine(w, weight_dtype="bf16").weight_dtype == "bf16"  # the argument wins
    assert _engine(w, weight_dtype="fp8").weight_dtype == "fp8"
    monkeypatch.setenv("DAB_WEIGHT_DTYPE", "fp8")
    assert _engine(w, weight_dtype="mxfp4").weight_dtype == "mxfp4"
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
    monkeypatch.setattr(serving, "setting", lambda name, default: "mxfp4" if name == "WEIGHT_DTYPE" else default)
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["weight_dtype"] == "mxfp4"
    seen.clear()
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu", weight_dtype="bf16")  # the argument wins over the setting
    assert seen["weight_dtype"] == "bf16"
