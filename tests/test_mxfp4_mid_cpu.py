"""``mxfp4_mid`` without a GPU: the CPU forms of ``ops.gemm_mid`` / ``ops.gemm_bt`` with ``w_scales``
(row-major codes and scales, ``ref.gemm_bt`` on the dequantised rows), the flag's parsing and refusals, and
a CPU model with the flag on (it changes nothing there)."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine
from django_assistant_bot_amd.models.configs import DecoderConfig
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel
from django_assistant_bot_amd.models.weights import random_decoder_weights
from django_assistant_bot_amd.ops import reference as ref

TOY = DecoderConfig("toy-w4-mid", vocab_size=256, hidden=128, layers=2, heads=4, kv_heads=2, intermediate=256,
                    max_position=256, bos_id=250, eos_ids=(251,), rope_scaling=None, rope_theta=10000.0)


def _weights(seed=3):
    return {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(TOY, dtype=torch.float32, seed=seed,
                                                                       interleave_mlp=True).items()}


@pytest.mark.parametrize("epi,res", [(ops.EPI_NONE, False), (ops.EPI_NONE, True), (ops.EPI_SWIGLU8, False)])
def test_cpu_gemm_with_w_scales_equals_the_reference_on_dequantised_rows(epi, res):
    M, N, K = 37, 256, 128
    g = torch.Generator().manual_seed(5)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    codes, scales = ops.weight_quantize_mxfp4(torch.randn(N, K, generator=g).to(torch.bfloat16))
    R = torch.randn(M, N, generator=g).to(torch.bfloat16) if res else None
    want = ref.gemm_bt(A, ops.weight_dequantize_mxfp4(codes, scales).to(A.dtype), None, R, epi)
    assert want.shape == (M, N // 2 if epi == ops.EPI_SWIGLU8 else N)
    assert torch.equal(ops.gemm_mid(A, codes, w_scales=scales, residual=R, epilogue=epi), want)
    assert torch.equal(ops.gemm_bt(A, codes, w_scales=scales, residual=R, epilogue=epi, shuffled=True), want)
    out = torch.empty_like(want)
    assert ops.gemm_bt(A, codes, w_scales=scales, residual=R, epilogue=epi, shuffled=True, out=out) is out
    assert torch.equal(out, want)


def test_cpu_gemm_with_w_scales_refusals():
    A = torch.zeros(4, 128, dtype=torch.bfloat16)
    codes, scales = ops.weight_quantize_mxfp4(torch.ones(256, 128, dtype=torch.bfloat16))
    for kw in (dict(shuffled=False), dict(shuffled=True, as_m=8), dict(shuffled=True, rows=torch.zeros(1, dtype=torch.int32)),
               dict(shuffled=True, bias=torch.zeros(256, dtype=torch.bfloat16)), dict(shuffled=True, out_f32=True),
               dict(shuffled=True, epilogue=ops.EPI_GELU), dict(shuffled=True, w_exps=scales[:, 0].contiguous())):
        with pytest.raises(ValueError):
            ops.gemm_bt(A, codes, w_scales=scales, **kw)
    with pytest.raises(ValueError):
        ops.gemm_mid(A, codes, w_scales=scales, variant=64)
    with pytest.raises(ValueError):
        ops.gemm_mid(A, codes, w_scales=scales, epilogue=ops.EPI_GELU)


def test_flag_needs_mxfp4_weights():
    w = _weights()
    for wd in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="mxfp4_mid needs weight_dtype='mxfp4'"):
            LlamaModel(TOY, dict(w), "cpu", interleaved_mlp=True, weight_dtype=wd, mxfp4_mid=True)
        with pytest.raises(ValueError, match="mxfp4_mid needs weight_dtype='mxfp4'"):
            LLMEngine(TOY, device="cpu", weights=dict(w), weight_dtype=wd, mxfp4_mid=True, num_blocks=8, max_batch=2)
    with pytest.raises(ValueError, match="fragment layout"):
        LlamaModel(TOY, dict(w), "cpu", interleaved_mlp=True, weight_dtype="mxfp4", mxfp4_mid=True, fragment_layout=False)
    m = LlamaModel(TOY, dict(w), "cpu", interleaved_mlp=True, weight_dtype="mxfp4", mxfp4_mid=True)
    assert m.mxfp4_mid and not m.mxfp4_weights_only and LlamaModel.MXFP4_MID_OFF == frozenset()
    assert not LlamaModel(TOY, dict(w), "cpu", interleaved_mlp=True, weight_dtype="mxfp4").mxfp4_mid


@pytest.mark.parametrize("env,want", [(None, False), ("", False), ("0", False), ("off", False), ("1", True), ("true", True),
                                      ("on", True), ("YES", True)])
def test_env_flag_parsing(env, want, monkeypatch):
    if env is None:
        monkeypatch.delenv("DAB_WEIGHT_MXFP4_MID", raising=False)
    else:
        monkeypatch.setenv("DAB_WEIGHT_MXFP4_MID", env)
    w = _weights()
    eng = LLMEngine(TOY, device="cpu", weights=dict(w), weight_dtype="mxfp4", num_blocks=8, max_batch=2)
    assert eng.mxfp4_mid is want and eng.model.mxfp4_mid is want and eng.stats["weight_mid_mxfp4"] is want
    # an argument wins over the environment
    eng = LLMEngine(TOY, device="cpu", weights=dict(w), weight_dtype="mxfp4", mxfp4_mid=not want, num_blocks=8, max_batch=2)
    assert eng.mxfp4_mid is (not want) and eng.stats["weight_mid_mxfp4"] is (not want)
    if want:  # the environment asks for it on a bf16 engine: refused like the argument
        with pytest.raises(ValueError, match="mxfp4_mid needs weight_dtype='mxfp4'"):
            LLMEngine(TOY, device="cpu", weights=dict(w), weight_dtype="bf16", num_blocks=8, max_batch=2)


def test_shared_model_decides_and_a_conflict_raises():
    w = _weights()
    e1 = LLMEngine(TOY, device="cpu", weights=dict(w), weight_dtype="mxfp4", mxfp4_mid=True, num_blocks=8, max_batch=2)
    e2 = LLMEngine(TOY, device="cpu", shared_model=e1.model, num_blocks=8, max_batch=2)
    assert e2.mxfp4_mid and e2.stats["weight_mid_mxfp4"] is True and e2.weight_dtype == "mxfp4"
    with pytest.raises(ValueError, match="mxfp4_mid=False conflicts"):
        LLMEngine(TOY, device="cpu", shared_model=e1.model, mxfp4_mid=False, num_blocks=8, max_batch=2)


def test_serving_reads_the_setting(monkeypatch):
    from django_assistant_bot_amd.engine import serving

    seen = {}

    class _Eng:
        def __init__(self, model, **kw):
            seen.update(kw)

    monkeypatch.setattr("django_assistant_bot_amd.engine.llm_engine.LLMEngine", _Eng)
    monkeypatch.setattr(serving, "LLMWorker", lambda eng: eng)
    monkeypatch.setattr(serving, "setting", lambda name, default=None: {"WEIGHT_MXFP4_MID": "on",
                                                                         "WEIGHT_DTYPE": "mxfp4"}.get(name, default))
    monkeypatch.setattr(serving, "_llm", {})
    serving.get_llm_worker("toy-setting", device="cpu")
    assert seen["mxfp4_mid"] is True and seen["mxfp4_weights_only"] is None and seen["weight_dtype"] == "mxfp4"


def test_cpu_model_with_the_flag_equals_the_model_without():
    w = _weights(8)
    outs = []
    for mid in (False, True):
        m = LlamaModel(TOY, dict(w), "cpu", interleaved_mlp=True, weight_dtype="mxfp4", mxfp4_mid=mid)
        T, bs = 40, 16
        ids = torch.arange(T, dtype=torch.int32) % TOY.vocab_size
        bt = torch.arange(3, dtype=torch.int32).view(1, 3)
        kv = KVCache(TOY.layers, 3, TOY.kv_heads, bs, TOY.head_dim, "cpu")
        meta = AttnMeta(decode=False, positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T),
                        block_tables=bt, ctx_lens=torch.tensor([T], dtype=torch.int32),
                        cu_q=torch.tensor([0, T], dtype=torch.int32), max_q=T)
        h = m.forward(ids, meta, kv)
        outs.append((h, m.logits(h), kv.k.clone(), kv.v.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(outs[0][0].float().abs().sum() > 0)
