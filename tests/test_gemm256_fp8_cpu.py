"""The FP8-weight arm of gemm256 and the FP8-only weight mode without a GPU: the CPU semantics of
``ops.gemm_bt(..., w_exps=)`` (the reference on the dequantised, unshuffled rows), the refusals that need no
launch, the operands of tests/gemm256_fp8_cases.py, and ``fp8_weights_only`` (argument, ``DAB_WEIGHT_FP8_ONLY``, the
``WEIGHT_FP8_ONLY`` serving setting), which a CPU model accepts and which changes nothing there."""
import pytest
import torch

import gemm256_fp8_cases as g8
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams, parse_flag
from django_assistant_bot_amd.models.configs import decoder_config
from django_assistant_bot_amd.models.llama import AttnMeta, Fp8Proj, KVCache, LlamaModel
from django_assistant_bot_amd.models.weights import random_decoder_weights
from django_assistant_bot_amd.ops import reference as ref


def test_case_operands_are_exact_and_far_apart():
    data, exps, dq = g8.weights(512, 384)
    e = exps.int()
    assert int(e.min()) == 1 and int(e.max()) == 254
    plain = torch.tensor([r not in g8.EXTREME and r + 1 not in g8.EXTREME for r in range(511)])
    assert int((e[1:] - e[:-1]).abs()[plain].min()) >= 16        # neighbouring rows
    assert int((e[8:] - e[:-8]).abs().min()) >= 1                # a gate row and its up row never share one
    assert bool(torch.isfinite(dq.float()).all()) and bool((dq.float().abs() > 0).any(1).all())
    a = g8.activations(257, 384)
    assert float(a.float().abs().min()) >= 2.0 ** -4 and float(a.float().abs().max()) <= 4.0
    assert torch.equal(ops.unshuffle_weights_fp8(ops.shuffle_weights_fp8(data, 8), 8), data)


@pytest.mark.parametrize("group", (1, 8))
def test_gemm_bt_on_cpu_tensors_is_the_reference_on_the_dequantised_rows(group):
    N, K, M = 512, 384, 37
    data, exps, dq = g8.weights(N, K)
    A = g8.activations(M, K)
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(1)).bfloat16()
    w8 = ops.shuffle_weights_fp8(data, group)
    kw = dict(shuffled=True, b_group=group, w_exps=exps)
    assert g8.same_bits(ops.gemm_bt(A, w8, **kw), ref.gemm_bt(A, dq))
    assert g8.same_bits(ops.gemm_bt(A, w8, residual=res, **kw), ref.gemm_bt(A, dq, None, res))
    want = ref.gemm_bt(A, dq, None, None, ops.EPI_SWIGLU8)
    assert g8.same_bits(ops.gemm_bt(A, w8, epilogue=ops.EPI_SWIGLU8, **kw), want)
    rows = torch.tensor([5, 5, 36, 0], dtype=torch.int32)
    assert g8.same_bits(ops.gemm_bt(A, w8, epilogue=ops.EPI_SWIGLU8, rows=rows, **kw), want[rows.long()])
    assert g8.same_bits(ops.gemm_bt(A[:9], w8, as_m=M, **kw), ref.gemm_bt(A[:9], dq))
    out = torch.empty(M, N, dtype=torch.bfloat16)
    assert ops.gemm_bt(A, w8, out=out, **kw) is out and g8.same_bits(out, ref.gemm_bt(A, dq))


def test_refusals_that_need_no_gpu():
    data, exps, _ = g8.weights(512, 384)
    A = g8.activations(8, 384)
    w8 = ops.shuffle_weights_fp8(data)
    bias = torch.zeros(512, dtype=torch.bfloat16)
    for kw in (dict(shuffled=False), dict(bias=bias), dict(epilogue=ops.EPI_GELU), dict(epilogue=ops.EPI_SWIGLU),
               dict(out_f32=True), dict(n=256), dict(row_group=torch.zeros(512, dtype=torch.int32)),
               dict(rows=torch.zeros(2, dtype=torch.int32), as_m=8)):
        a = dict(shuffled=True, w_exps=exps)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.gemm_bt(A, w8, **a)
    # a wide FP8 candidate batch is opt-in: without ``wide`` more than one scan launch is still refused
    assert ops.fp8_scan_max_m(768) == 96
    assert parse_flag("1") and parse_flag("True") and parse_flag(" on ") and parse_flag(True)
    assert not parse_flag("0") and not parse_flag("") and not parse_flag(None) and not parse_flag("off")


# ------------------------------------------------------------------------------------------ the FP8-only mode

CFG = decoder_config("tiny-llama")


def _weights(seed=3):
    return {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(CFG, dtype=torch.float32, seed=seed,
                                                                       interleave_mlp=True).items()}


def test_cpu_model_accepts_the_mode_and_computes_the_same():
    w = _weights()
    m1 = LlamaModel(CFG, dict(w), "cpu", interleaved_mlp=True, weight_dtype="fp8", fp8_weights_only=True)
    m2 = LlamaModel(CFG, dict(w), "cpu", interleaved_mlp=True, weight_dtype="fp8")
    assert m1.fp8_weights_only and not m2.fp8_weights_only and not m1.frag
    assert not isinstance(m1.layers[0].qkv_w, Fp8Proj) and m1.projection_bytes() == m2.projection_bytes()
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
    with pytest.raises(ValueError, match="weight_dtype='fp8'"):
        LlamaModel(CFG, dict(w), "cpu", fp8_weights_only=True)
    with pytest.raises(ValueError, match="weight_dtype='fp8'"):
        LlamaModel(CFG, dict(w), "cpu", weight_dtype="bf16", fp8_weights_only=True)
    with pytest.raises(ValueError, match="tensor parallelism"):
        LlamaModel(CFG, dict(w), "cpu", weight_dtype="fp8", fp8_weights_only=True, tp_size=2, tp_rank=0)
    with pytest.raises(ValueError, match="fragment"):
        LlamaModel(CFG, dict(w), "cpu", weight_dtype="fp8", fp8_weights_only=True, fragment_layout=False)

    class NoStream(LlamaModel):
        fp8_stream = False

    class SomeOff(LlamaModel):
        FP8_STREAM_OFF = frozenset({("qkv", 13)})

    for cls in (NoStream, SomeOff):
        with pytest.raises(ValueError, match="fp8_stream"):
            cls(CFG, dict(w), "cpu", weight_dtype="fp8", fp8_weights_only=True)
        cls(CFG, dict(w), "cpu", weight_dtype="fp8")  # (the two-copy mode keeps both switches)


def _engine(weights, **kw):
    args = dict(device="cpu", weights=dict(weights), max_batch=8, block_size=16, num_blocks=64, max_prefill_tokens=256,
                use_graphs=False)
    args.update(kw)
    return LLMEngine(CFG, **args)


def test_engine_option_stats_and_tokens():
    w = _weights()
    greedy = SamplingParams(max_new_tokens=6, do_sample=False, temperature=0.0, ignore_eos=True)
    toks = []
    for eng in (_engine(w, weight_dtype="fp8", fp8_weights_only=True), _engine(w, weight_dtype="fp8")):
        rids = [eng.add_request(list(range(5, 5 + n)), greedy) for n in (20, 9)]
        while eng.has_unfinished():
            eng.step()
        toks.append([eng.pop_output(r).token_ids for r in rids])
    assert toks[0] == toks[1]
    e1, e2, e16 = _engine(w, weight_dtype="fp8", fp8_weights_only=True), _engine(w, weight_dtype="fp8"), _engine(w)
    assert e1.fp8_weights_only and e1.model.fp8_weights_only and e1.stats["weight_bf16_copy"] is False
    assert not e2.fp8_weights_only and e2.stats["weight_bf16_copy"] is True and e16.stats["weight_bf16_copy"] is True
    bf16 = sum(2 * v.numel() for k, v in w.items() if k.endswith(("qkv_w", "o_w", "gate_up_w", "down_w")))
    assert e16.stats["weight_bytes"] == bf16 == e1.stats["weight_bytes"]  # (CPU: dequantised row-major weights)
    assert isinstance(e1.stats["weight_bytes"], int)
    second = _engine(w, shared_model=e1.model)
    assert second.fp8_weights_only and second.stats["weight_bf16_copy"] is False
    with pytest.raises(ValueError, match="fp8_weights_only"):
        _engine(w, shared_model=e1.model, fp8_weights_only=False)
    with pytest.raises(ValueError, match="fp8_weights_only"):
        _engine(w, fp8_weights_only=True)
    with pytest.raises(ValueError, match="fp8_weights_only"):
        _engine(w, weight_dtype="bf16", fp8_weights_only=True)
    with pytest.raises(ValueError, match="tensor parallelism"):
        _engine(w, weight_dtype="fp8", fp8_weights_only=True, tp_size=2)


def test_environment_variable(monkeypatch):
    w = _weights()
    monkeypatch.setenv("DAB_WEIGHT_DTYPE", "fp8")
    monkeypatch.setenv("DAB_WEIGHT_FP8_ONLY", "1")
    assert _engine(w).fp8_weights_only and _engine(w).weight_dtype == "fp8"
    assert not _engine(w, fp8_weights_only=False).fp8_weights_only  # the argument wins
    monkeypatch.setenv("DAB_WEIGHT_FP8_ONLY", "0")
    assert not _engine(w).fp8_weights_only
    monkeypatch.setenv("DAB_WEIGHT_FP8_ONLY", "true")
    monkeypatch.delenv("DAB_WEIGHT_DTYPE")
    with pytest.raises(ValueError, match="fp8_weights_only"):  # the variable without FP8 weights
        _engine(w)
    monkeypatch.delenv("DAB_WEIGHT_FP8_ONLY")
    assert not _engine(w).fp8_weights_only


def test_serving_setting_reaches_the_engine(monkeypatch):
    from django_assistant_bot_amd.engine import llm_engine, serving

    seen = {}

    class _Eng:
        def __init__(self, model, **kw):
            seen.update(kw)

    monkeypatch.setattr(llm_engine, "LLMEngine", _Eng)
    monkeypatch.setattr(serving, "LLMWorker", lambda e: e)
    values = {"WEIGHT_DTYPE": "fp8", "WEIGHT_FP8_ONLY": "1"}
    monkeypatch.setattr(serving, "setting", lambda name, default: values.get(name, default))
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["weight_dtype"] == "fp8" and seen["fp8_weights_only"] is True
    seen.clear()
    values["WEIGHT_FP8_ONLY"] = False
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["fp8_weights_only"] is False
    seen.clear()
    monkeypatch.setattr(serving, "setting", lambda name, default: default)
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu")
    assert seen["fp8_weights_only"] is None  # the engine then reads DAB_WEIGHT_FP8_ONLY, else off
    seen.clear()
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("tiny-llama", device="cpu", fp8_weights_only=True)
    assert seen["fp8_weights_only"] is True
