"""``mxfp4_weights_only`` without a GPU: the CPU form of ``ops.weight_dequant_mxfp4``, the refusals of
model and engine, the plumbing of the option (argument, ``DAB_WEIGHT_MXFP4_ONLY``, the serving setting,
``shared_model``) and the statistics.  On the CPU the option changes nothing the model computes."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams
from django_assistant_bot_amd.models.configs import decoder_config
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel, Mxfp4Proj
from django_assistant_bot_amd.models.weights import random_decoder_weights

SCALE_BYTES = (2, 3, 126, 127, 128, 251, 252)
PROJ = ("qkv_w", "o_w", "gate_up_w", "down_w")


def _raw(N, K, seed):
    """Row-major codes [N, K/2] over all 16 values and scale bytes [N, K/32] from both ends of the range."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scales = torch.tensor(SCALE_BYTES, dtype=torch.uint8)[torch.randint(0, len(SCALE_BYTES), (N, K // 32), generator=g)]
    return codes, scales


# ---------------------------------------------------------------------------------------------------- op


@pytest.mark.parametrize("N,K,group", [(16, 128, 1), (48, 256, 1), (128, 384, 8), (256, 128, 8)])
def test_cpu_op_equals_the_reference_composition(N, K, group):
    codes, scales = _raw(N, K, N + K)
    want = ops.shuffle_weights(ops.weight_dequantize_mxfp4(codes, scales), group)
    assert bool(torch.isfinite(want.float()).all()) and bool((want != 0).any())
    out = torch.full((N * K + 2048,), -7.0, dtype=torch.bfloat16)
    got = ops.weight_dequant_mxfp4(ops.shuffle_weights_mxfp4(codes, group), ops.shuffle_scales_mxfp4(scales), out, group)
    assert got.shape == (N, K) and got.data_ptr() == out.data_ptr()
    assert torch.equal(got, want) and torch.equal(out[:N * K].view(N, K), want)
    assert bool((out[N * K:] == -7.0).all())  # nothing past N K elements


def test_cpu_op_refuses_bad_arguments():
    N, K = 128, 256
    codes, scales = _raw(N, K, 1)
    c4, sc = ops.shuffle_weights_mxfp4(codes), ops.shuffle_scales_mxfp4(scales)
    out = torch.zeros(N * K, dtype=torch.bfloat16)
    ops.weight_dequant_mxfp4(c4, sc, out)
    bad = [
        (c4[:, :96].contiguous(), sc[:, :6].contiguous(), out, 1),  # K % 128
        (c4[:24].contiguous(), sc[:24].contiguous(), out, 1),  # N % 16
        (c4[:64].contiguous(), sc[:64].contiguous(), out, 8),  # N % (16 group)
        (c4.to(torch.int8), sc, out, 1), (c4, sc.to(torch.int32), out, 1), (c4, sc, out.float(), 1),  # dtypes
        (c4, sc[:-16], out, 1), (c4, sc.reshape(-1), out, 1),  # scales of another shape
        (c4, sc, out[:-1], 1),  # out too small
        (c4.t().contiguous().t(), sc, out, 1), (c4, sc, out.view(N, K)[:, ::2], 1),  # not contiguous
        (c4, sc, out, 0),
    ]
    for c, s, o, g in bad:
        before = o.clone()
        with pytest.raises(ValueError):
            ops.weight_dequant_mxfp4(c, s, o, g)
        assert torch.equal(o, before)


# ------------------------------------------------------------------------------------------------- model

CFG = decoder_config("tiny-llama")


def _weights(seed=3):
    return {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(CFG, dtype=torch.float32, seed=seed,
                                                                       interleave_mlp=True).items()}


def test_cpu_model_accepts_the_mode_and_computes_the_same():
    w = _weights()
    m1 = LlamaModel(CFG, dict(w), "cpu", interleaved_mlp=True, weight_dtype="mxfp4", mxfp4_weights_only=True)
    m2 = LlamaModel(CFG, dict(w), "cpu", interleaved_mlp=True, weight_dtype="mxfp4")
    assert m1.mxfp4_weights_only and not m2.mxfp4_weights_only and not m1.frag
    assert not isinstance(m1.layers[0].qkv_w, Mxfp4Proj) and m1.projection_bytes() == m2.projection_bytes()
    assert m1.mxfp4_scratch_bytes() == 0 == m2.mxfp4_scratch_bytes()
    T = 21
    ids = torch.arange(5, 5 + T, dtype=torch.int32)
    outs = []
    for m in (m1, m2):
        kv = KVCache(CFG.layers, 4, CFG.kv_heads, 16, CFG.head_dim, "cpu", dtype=torch.float32)
        meta = AttnMeta(decode=False, positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T),
                        block_tables=torch.arange(4, dtype=torch.int32)[None], ctx_lens=torch.tensor([T], dtype=torch.int32),
                        cu_q=torch.tensor([0, T], dtype=torch.int32), max_q=T)
        h = m.forward(ids, meta, kv)
        outs.append((h, m.logits(h[-1:]), kv.k.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_model_refusals():
    w = _weights()
    for wd in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="mxfp4_weights_only needs weight_dtype='mxfp4'"):
            LlamaModel(CFG, dict(w), "cpu", weight_dtype=wd, mxfp4_weights_only=True)
    with pytest.raises(ValueError, match="mxfp4_weights_only needs weight_dtype='mxfp4'"):
        LlamaModel(CFG, dict(w), "cpu", mxfp4_weights_only=True)
    with pytest.raises(ValueError, match="tensor parallelism"):
        LlamaModel(CFG, dict(w), "cpu", weight_dtype="mxfp4", mxfp4_weights_only=True, tp_size=2, tp_rank=0)
    with pytest.raises(ValueError, match="mxfp4_weights_only needs the fragment layout"):
        LlamaModel(CFG, dict(w), "cpu", weight_dtype="mxfp4", mxfp4_weights_only=True, fragment_layout=False)
    with pytest.raises(ValueError, match="mutually exclusive"):
        LlamaModel(CFG, dict(w), "cpu", weight_dtype="fp8", fp8_weights_only=True, mxfp4_weights_only=True)
    with pytest.raises(ValueError, match="fp8_weights_only"):  # (the refusal the two-copy mode already had)
        LlamaModel(CFG, dict(w), "cpu", weight_dtype="mxfp4", fp8_weights_only=True, mxfp4_weights_only=True)


def test_proj_without_a_bf16_copy():
    """``Mxfp4Proj.from_rows(bf16_copy=False)``: shape from the codes, bytes and regroup without ``w``."""
    N, K = 128, 256
    codes, scales = _raw(N, K, 9)
    two, one = Mxfp4Proj.from_rows(codes, scales, 8), Mxfp4Proj.from_rows(codes, scales, 8, bf16_copy=False)
    assert one.w is None and two.w is not None
    assert tuple(one.shape) == tuple(two.shape) == (N, K) == tuple(two.w.shape)
    assert one.nbytes() == N * K // 2 + N * K // 32 and two.nbytes() == one.nbytes() + 2 * N * K
    assert torch.equal(one.data, two.data) and torch.equal(one.scales, two.scales)
    ptr = one.data.data_ptr()
    one.regroup(1)
    two.regroup(1)
    assert one.group == 1 and one.w is None and one.data.data_ptr() == ptr
    assert torch.equal(one.data, two.data) and torch.equal(one.data, ops.shuffle_weights_mxfp4(codes, 1))
    out = torch.empty(N * K, dtype=torch.bfloat16)
    assert torch.equal(ops.weight_dequant_mxfp4(one.data, one.scales, out, one.group), two.w)


# ------------------------------------------------------------------------------------------------ engine


def _engine(weights, **kw):
    args = dict(device="cpu", weights=dict(weights), max_batch=8, block_size=16, num_blocks=64, max_prefill_tokens=256,
                use_graphs=False)
    args.update(kw)
    return LLMEngine(CFG, **args)


def test_engine_option_stats_and_tokens():
    w = _weights()
    greedy = SamplingParams(max_new_tokens=6, do_sample=False, temperature=0.0, ignore_eos=True)
    toks = []
    for eng in (_engine(w, weight_dtype="mxfp4", mxfp4_weights_only=True), _engine(w, weight_dtype="mxfp4")):
        rids = [eng.add_request(list(range(5, 5 + n)), greedy) for n in (20, 9)]
        while eng.has_unfinished():
            eng.step()
        toks.append([eng.pop_output(r).token_ids for r in rids])
    assert toks[0] == toks[1]
    e1, e2, e16 = _engine(w, weight_dtype="mxfp4", mxfp4_weights_only=True), _engine(w, weight_dtype="mxfp4"), _engine(w)
    assert e1.mxfp4_weights_only and e1.model.mxfp4_weights_only and e1.stats["weight_bf16_copy"] is False
    assert not e2.mxfp4_weights_only and e2.stats["weight_bf16_copy"] is True and e16.stats["weight_bf16_copy"] is True
    assert e1.stats["weight_bits"] == e2.stats["weight_bits"] == 4
    bf16 = sum(2 * v.numel() for k, v in w.items() if k.endswith(PROJ))
    assert e16.stats["weight_bytes"] == bf16 == e1.stats["weight_bytes"]  # (CPU: dequantised row-major weights)
    for e in (e1, e2, e16):  # (no scratch on the CPU; a number like every other entry)
        assert e.stats["weight_scratch_bytes"] == 0 and isinstance(e.stats["weight_scratch_bytes"], int)
    second = _engine(w, shared_model=e1.model)
    assert second.mxfp4_weights_only and second.weight_dtype == "mxfp4" and second.stats["weight_bf16_copy"] is False
    assert not _engine(w, shared_model=e2.model).mxfp4_weights_only
    with pytest.raises(ValueError, match="mxfp4_weights_only.*conflicts"):
        _engine(w, shared_model=e1.model, mxfp4_weights_only=False)
    with pytest.raises(ValueError, match="mxfp4_weights_only.*conflicts"):
        _engine(w, shared_model=e2.model, mxfp4_weights_only=True)


def test_engine_refusals():
    w = _weights()
    with pytest.raises(ValueError, match="mxfp4_weights_only needs weight_dtype='mxfp4'"):
        _engine(w, mxfp4_weights_only=True)
    for wd in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="mxfp4_weights_only needs weight_dtype='mxfp4'"):
            _engine(w, weight_dtype=wd, mxfp4_weights_only=True)
    with pytest.raises(ValueError, match="tensor parallelism"):
        _engine(w, weight_dtype="mxfp4", mxfp4_weights_only=True, tp_size=2)
    with pytest.raises(ValueError, match="mutually exclusive"):
        _engine(w, weight_dtype="fp8", fp8_weights_only=True, mxfp4_weights_only=True)
    with pytest.raises(ValueError, match="fp8_weights_only"):
        _engine(w, weight_dtype="mxfp4", fp8_weights_only=True, mxfp4_weights_only=True)


def test_environment_variable(monkeypatch):
    w = _weights()
    monkeypatch.setenv("DAB_WEIGHT_DTYPE", "mxfp4")
    monkeypatch.setenv("DAB_WEIGHT_MXFP4_ONLY", "1")
    assert _engine(w).mxfp4_weights_only and _engine(w).weight_dtype == "mxfp4"
    assert not _engine(w, mxfp4_weights_only=False).mxfp4_weights_only  # the argument wins
    monkeypatch.setenv("DAB_WEIGHT_MXFP4_ONLY", "0")
    assert not _engine(w).mxfp4_weights_only
    monkeypatch.setenv("DAB_WEIGHT_MXFP4_ONLY", "true")
    monkeypatch.delenv("DAB_WEIGHT_DTYPE")
    with pytest.raises(ValueError, match="mxfp4_weights_only"):  # the variable without MXFP4 weights
        _engine(w)
    monkeypatch.delenv("DAB_WEIGHT_MXFP4_ONLY")
    assert not _engine(w).mxfp4_weights_only


def test_serving_setting_reaches_the_engine(monkeypatch):
    from django_assistant_bot_amd.engine import llm_engine, serving

    seen = {}

    class _Eng:
        def __init__(self, model, **kw):
            seen.update(kw)

    monkeypatch.setattr(llm_engine, "LLMEngine", _Eng)
    monkeypatch.setattr(serving, "LLMWorker", lambda e: e)
    values = {"WEIGHT_DTYPE": "mxfp4", "WEIGHT_MXFP4_ONLY": "1"}
    monkeypatch.setattr(serving, "setting", lambda name, default: values.get(name, default))
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["weight_dtype"] == "mxfp4" and seen["mxfp4_weights_only"] is True and seen["fp8_weights_only"] is None
    seen.clear()
    values["WEIGHT_MXFP4_ONLY"] = False
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["mxfp4_weights_only"] is False
    seen.clear()
    monkeypatch.setattr(serving, "setting", lambda name, default: default)
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["mxfp4_weights_only"] is None  # the engine then reads DAB_WEIGHT_MXFP4_ONLY, else off
    seen.clear()
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu", mxfp4_weights_only=True)  # the argument wins
    assert seen["mxfp4_weights_only"] is True
