"""Opt-in MXFP4 projection weights (W4A16) on the GPU: the MXFP4 arm of the streaming decode GEMM
(``ops.stream_gemm(..., w_scales=...)``), ``LlamaModel(weight_dtype="mxfp4")`` and
``LLMEngine(weight_dtype="mxfp4")``.

Every dequantised weight (an e2m1 code times a power of two) is bf16-exact and the kernel converts the
codes to exactly those values before the bf16 MFMA, so the MXFP4 kernel must EQUAL the bf16 kernel run
on the dequantised weights; the one-hot tests pin the nibble order, the layouts and the scale bytes
without the bf16 kernel and without the quantiser.  Every comparison is ``torch.equal``."""
import math

import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.models import llama
from django_assistant_bot_amd.models.configs import DecoderConfig
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel, Mxfp4Proj
from django_assistant_bot_amd.models.weights import random_decoder_weights

pytestmark = pytest.mark.gpu

DEV = "cuda"
# what the decoder can dispatch for qkv / o / gate_up / down: _stream_cfg (30, 31, 13, 10, 27), the
# wide gate_up tiling (20) and the small-batch residual producers (32).  Cfg 27 (batches of 129..256)
# has two k-groups: a wave reads half of every 128-deep fragment with 8-byte lane loads.
MX_CFGS = [10, 13, 20, 27, 30, 31, 32]
PROJ = ("qkv_w", "o_w", "gate_up_w", "down_w")


@pytest.fixture
def ring(request):
    """The MXFP4 arm's ring depth mode for one test (0: the bf16 configuration's stages, 1: twice that)."""
    nat = ops.native()
    old = nat.stream_gemm_mxfp4_deep()
    nat.stream_gemm_mxfp4_set_deep(request.param)
    yield request.param
    nat.stream_gemm_mxfp4_set_deep(old)


def _weights(N, K, seed):
    """bf16 [N, K] with block magnitudes 2^-10 .. 2^2 within every row, both signs, one zero row (row 3)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K // 32, 32, generator=g) * torch.exp2(torch.randint(-10, 3, (N, K // 32, 1), generator=g).float())
    w = w.reshape(N, K)
    w[3] = 0
    return w.bfloat16()


def _quantised(N, K, seed, group=1):
    """(MXFP4 fragment copy, scale copy, bf16 fragment copy of the dequantised values, dequantised [N, K])."""
    codes, scales = ops.weight_quantize_mxfp4(_weights(N, K, seed))
    dq = ops.weight_dequantize_mxfp4(codes, scales)
    return (ops.shuffle_weights_mxfp4(codes, group).to(DEV), ops.shuffle_scales_mxfp4(scales).to(DEV),
            ops.shuffle_weights(dq, group).to(DEV), dq)


def test_mxfp4_ok_names_the_dispatched_configurations():
    nat = ops.native()
    assert [c for c in range(64) if nat.stream_gemm_mxfp4_ok(c)] == MX_CFGS
    assert not nat.stream_gemm_mxfp4_ok(-1) and not nat.stream_gemm_mxfp4_ok(28)  # (the LM head's is not)
    m = LlamaModel
    assert {m.STREAM_CFG_M16, m.STREAM_CFG_M32, m.STREAM_CFG_M64, m.STREAM_CFG_M128, m.STREAM_CFG_M256,
            m.STREAM_WIDE["gate_up"], m.STREAM_CFG_RES16} == set(MX_CFGS)
    for c in MX_CFGS:
        assert nat.stream_gemm_shuffled(c) and nat.stream_gemm_fp8_ok(c)
        for deep in (0, 1):
            old = nat.stream_gemm_mxfp4_deep()
            nat.stream_gemm_mxfp4_set_deep(deep)
            assert nat.stream_gemm_mxfp4_nwin(c) == nat.stream_gemm_fp8_nwin(c) // (2 if nat.stream_gemm_fp8_deep() else 1) * (deep + 1)
            nat.stream_gemm_mxfp4_set_deep(old)
    assert nat.stream_gemm_mxfp4_nwin(28) == 0


# ----------------------------------------------------------------------------------------- kernel: one-hot


def _raw_weights(N, K):
    """Codes and scale bytes written down, not quantised: all 16 codes cycle along K (shifted per row,
    -0 included), the scale bytes cover both ends of the allowed range, 126-128 and a spread."""
    n = (torch.arange(K)[None, :] + 5 * torch.arange(N)[:, None]) % 16
    codes = (n[:, 0::2] | (n[:, 1::2] << 4)).to(torch.uint8)
    pool = torch.tensor([2, 3, 126, 127, 128, 251, 252] + list(range(5, 250, 7)) + [200])  # (43: odd, rows differ)
    scales = pool[torch.arange(N * (K // 32)) % len(pool)].view(N, K // 32).to(torch.uint8)
    return codes, scales


@pytest.mark.parametrize("ring", [0, 1], indirect=True)
@pytest.mark.parametrize("cfg", MX_CFGS)
def test_one_hot_rows_read_every_code_under_every_scale(cfg, ring):
    """X rows with a single 1.0: the output row is column k of the dequantised weights, exactly (one
    exact product, zeros added).  A wrong nibble order, lane map, scale row or block, or slice offset fails."""
    nat = ops.native()
    N, K, S = 2 * nat.stream_gemm_bn(cfg), 512, 2
    kc = K // S
    codes, scales = _raw_weights(N, K)
    assert {2, 3, 126, 127, 128, 251, 252} <= set(scales.flatten().tolist()) and len(set(scales.flatten().tolist())) > 30
    dq = ops.weight_dequantize_mxfp4(codes, scales)
    assert bool(torch.isfinite(dq.float()).all())
    w4, sc = ops.shuffle_weights_mxfp4(codes).to(DEV), ops.shuffle_scales_mxfp4(scales).to(DEV)
    # (M <= 16 on the smallest configurations: two sets of 16 rows)
    # every (chunk of a 128-deep fragment, lane quadrant), in all four fragments, both nibbles of a byte
    grid = [128 * (i % 4) + 32 * (i // 4) + 8 * (i % 4) + (3 * i + i // 4) % 8 for i in range(16)]
    assert {((k % 128) // 32, (k % 32) // 8) for k in grid} == {(c, q) for c in range(4) for q in range(4)}
    assert {k & 1 for k in grid} == {0, 1} and {k // 128 for k in grid} == {0, 1, 2, 3}
    # first / last k of a fragment, of a K-slice and of K, both nibbles around each
    edges = [0, 1, 31, 32, 126, 127, 128, kc - 2, kc - 1, kc, kc + 1, kc + 127, K - 128, K - 33, K - 2, K - 1]
    for ks in (grid, edges):
        x = torch.zeros((len(ks), K), dtype=torch.bfloat16)
        x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
        x = x.to(DEV)
        want = dq[:, ks].t().contiguous()  # [M, N]
        assert bool((want < 0).any()) and bool((want > 0).any())
        y = ops.stream_gemm(x, w4, w_scales=sc, cfg=cfg, nt=True)
        assert y.dtype == torch.bfloat16 and torch.equal(y.cpu(), want)
        slabs = ops.stream_gemm(x, w4, w_scales=sc, cfg=cfg, nt=False, splits=S).cpu()
        assert slabs.dtype == torch.float32 and slabs.shape == (S, len(ks), N)
        for m, k in enumerate(ks):
            own = k // kc
            assert torch.equal(slabs[own, m], want[m].float()), (m, k)
            assert not bool(slabs[1 - own, m].any()), (m, k)
    # all 16 codes under all the scale bytes were read: every (code, scale byte) pair of the 32 columns
    seen = {(int(c), int(s)) for k in grid + edges
            for c, s in zip(((torch.arange(N) * 5 + k) % 16).tolist(), scales[:, k // 32].tolist())}
    assert {c for c, _ in seen} == set(range(16)) and {s for _, s in seen} >= {2, 3, 126, 127, 128, 251, 252}


# ------------------------------------------------------------------- kernel: bit equality with the bf16 kernel


def _forms(x, w, sc, cfg, S, res, **kw):
    """Every output form of one (x, weights) pair (the forms of the FP8 test); ``sc`` None: the bf16 kernel."""
    a = dict(cfg=cfg, nt=True, w_scales=sc, **kw)
    eps = 1e-5
    return {
        "plain": ops.stream_gemm(x, w, **a),
        "residual": ops.stream_gemm(x, w, residual=res, **a),
        "swiglu8": ops.stream_gemm(x, w, epilogue=ops.EPI_SWIGLU8, **a),
        "slabs32": ops.stream_gemm(x, w, splits=S, **a),
        "slabs16": ops.stream_gemm(x, w, splits=S, slab_dtype=torch.bfloat16, **a),
        "norm_slabs32": ops.stream_gemm(x, w, splits=S, norm_eps=eps, **a),
        "norm_swiglu8": ops.stream_gemm(x, w, epilogue=ops.EPI_SWIGLU8, norm_eps=eps, **a),
        "plain_cached_loads": ops.stream_gemm(x, w, **{**a, "nt": False}),
    }


@pytest.mark.parametrize("ring", [0, 1], indirect=True)
@pytest.mark.parametrize("cfg", MX_CFGS)
def test_bit_equal_to_the_bf16_kernel_on_the_dequantised_weights(cfg, ring):
    """stream_gemm(x, w4, w_scales=sc) == stream_gemm(x, shuffle_weights(dq)) for every form the
    configuration serves, at M = 1, 16, 17, an odd value and the maximum, and K-slices shorter than
    the weight ring (clamped spare loads), whole multiples of it and with tail stages."""
    nat = ops.native()
    bn, max_m = nat.stream_gemm_bn(cfg), nat.stream_gemm_max_m(cfg)
    nwin = nat.stream_gemm_mxfp4_nwin(cfg)
    assert nwin > 0 and nat.stream_gemm_mxfp4_deep() == ring
    S = 2
    Ms = sorted({m for m in (1, 16, 17, 5 if max_m <= 32 else 2 * (max_m // 3) + 1, max_m) if m <= max_m})
    g = torch.Generator().manual_seed(cfg)
    for nst in (2, nwin, 2 * nwin, nwin + 1):  # stages per K-slice
        K = 128 * nst * S
        for group, N in ((1, 2 * bn), (8, math.lcm(2 * bn, 128))):
            if group == 8 and nst != nwin + 1:
                continue  # (the grouped copy: one K, every form and M)
            w4, sc, w16, _ = _quantised(N, K, 100 * cfg + nst, group)
            for M in Ms:
                x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
                res = torch.randn(M, N, generator=g).bfloat16().to(DEV)
                got = _forms(x, w4, sc, cfg, S, res, w_group=group)
                want = _forms(x, w16, None, cfg, S, res, w_group=group)
                for name in want:
                    assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape
                    assert torch.equal(got[name], want[name]), (cfg, ring, nst, group, M, name)
                assert bool(want["plain"].float().abs().sum() > 0)


# ------------------------------------------------------------------------------------ kernel: invalid launches


def test_invalid_launches_are_refused_without_a_launch(monkeypatch):
    nat = ops.native()
    cfg = 13
    N, K = 2 * nat.stream_gemm_bn(cfg), 256
    w4, sc, w16, _ = _quantised(N, K, 5)
    x = torch.randn(4, K).bfloat16().to(DEV)
    ok = ops.stream_gemm(x, w4, w_scales=sc, cfg=cfg)
    launched = []
    real = nat.stream_gemm_mxfp4
    monkeypatch.setattr(nat, "stream_gemm_mxfp4", lambda *a, **k: launched.append(1) or real(*a, **k))
    assert torch.equal(ops.stream_gemm(x, w4, w_scales=sc, cfg=cfg), ok) and launched == [1]
    with pytest.raises(ValueError, match="K % 128"):
        ops.stream_gemm(x[:, :192].contiguous(), w4[:, :96].contiguous(), w_scales=sc[:, :6].contiguous(), cfg=cfg)
    with pytest.raises(ValueError, match="bf16 operands"):  # codes without their scales
        ops.stream_gemm(x, w4, cfg=cfg)
    for bad in (sc[:-1], sc[:, :-1], sc.reshape(-1), sc.to(torch.int32), sc.cpu(), sc.float(), sc.t().contiguous().t()):
        with pytest.raises(ValueError, match="w_scales"):
            ops.stream_gemm(x, w4, w_scales=bad, cfg=cfg)
    odd = torch.empty(sc.numel() + 4, dtype=torch.uint8, device=DEV)[2:2 + sc.numel()].view(sc.shape).copy_(sc)
    with pytest.raises(ValueError, match="4-byte aligned"):
        ops.stream_gemm(x, w4, w_scales=odd, cfg=cfg)
    with pytest.raises(ValueError, match="uint8 fragment copy"):
        ops.stream_gemm(x, w16, w_scales=sc, cfg=cfg)
    off = torch.empty(w4.numel() + 16, dtype=torch.uint8, device=DEV)[8:8 + w4.numel()].view(w4.shape).copy_(w4)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.stream_gemm(x, off, w_scales=sc, cfg=cfg)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.stream_gemm(x, w4, w_scales=sc, w_exps=torch.full((N,), 127, dtype=torch.uint8, device=DEV), cfg=cfg)
    with pytest.raises(ValueError):  # x of another width
        ops.stream_gemm(x[:, :128].contiguous(), w4, w_scales=sc, cfg=cfg)
    for c in (11, 28, 17):  # a fragment-layout cfg without an MXFP4 arm, the LM head's, an ablation
        assert not nat.stream_gemm_mxfp4_ok(c)
        with pytest.raises(ValueError, match="no MXFP4-weight instantiation"):
            ops.stream_gemm(x, w4, w_scales=sc, cfg=c)
    assert launched == [1]
    monkeypatch.undo()
    # the entry point itself: hipErrorInvalidValue before any launch
    out = torch.full((4, N), 7.0, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def raw(K_=K, w=w4.data_ptr(), scales=sc.data_ptr(), cfg_=cfg):
        nat.stream_gemm_mxfp4(x.data_ptr(), K, w, scales, out.data_ptr(), N, 0, 0, 4, N, K_, 1, 0, s, 1, cfg_)

    for kw in (dict(K_=K + 64), dict(scales=0), dict(scales=sc.data_ptr() + 2), dict(w=0), dict(w=w4.data_ptr() + 8),
               dict(cfg_=11), dict(cfg_=28), dict(cfg_=99)):
        with pytest.raises(RuntimeError, match="stream_gemm_mxfp4"):
            raw(**kw)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    raw()
    assert torch.equal(out, ok)


# -------------------------------------------------------------------------------------------------- model

# every projection streams at decode batches <= 128 and in a 64-token prefill: N % 128 == 0 (cfg 30 /
# 13 / 10), gate_up's 1792 rows are also whole 112-row tiles (cfg 20 at M 65..128), K % 128 == 0
TOY = DecoderConfig("toy-w4", vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, intermediate=896,
                    max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)


def _toy_weights(seed):
    return {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(TOY, dtype=torch.float32, seed=seed,
                                                                       interleave_mlp=True).items()}


def _dequantised(weights):
    return {k: (ops.weight_dequantize_mxfp4(*ops.weight_quantize_mxfp4(v)) if k.endswith(PROJ) else v)
            for k, v in weights.items()}


@pytest.fixture(scope="module")
def toy_models():
    w = _toy_weights(6)
    m4 = LlamaModel(TOY, dict(w), DEV, interleaved_mlp=True, weight_dtype="mxfp4")
    m16 = LlamaModel(TOY, _dequantised(w), DEV, interleaved_mlp=True)
    assert m4.frag and m16.frag and m4.proj_group == m16.proj_group and m4.proj_group["gate_up"] == 8
    for L4, L16 in zip(m4.layers, m16.layers):
        for n in PROJ:
            p4, p16 = getattr(L4, n), getattr(L16, n)
            assert isinstance(p4, Mxfp4Proj) and p4.data.dtype == torch.uint8 and p4.scales.dtype == torch.uint8
            assert tuple(p4.shape) == tuple(p16.shape) and p4.data.shape == (p16.shape[0], p16.shape[1] // 2)
            assert p4.scales.shape == (p16.shape[0], p16.shape[1] // 32)
            assert torch.equal(p4.w, p16)  # the bf16 copy holds the dequantised values
            assert p4.nbytes() == p16.numel() * 2 + p16.numel() // 2 + p16.numel() // 32
    assert m4.projection_bytes() == sum(getattr(L, n).nbytes() for L in m4.layers for n in PROJ)
    assert torch.equal(m4.lm_head, m16.lm_head) and m4.lm_head.dtype == torch.bfloat16
    return m4, m16


def _streams(model, M):
    """{projection: stream_gemm cfg} the model chooses at M rows."""
    L = model.layers[0]
    return {n: model._stream_choice(n[:-2], M, *getattr(L, n).shape)[0] for n in PROJ}


class _Calls:
    """Counts ops.stream_gemm calls of the model by weight type."""

    def __init__(self, monkeypatch):
        self.mx = self.bf16 = 0
        real = ops.stream_gemm

        def spy(x, w, *a, **k):
            assert k.get("w_exps") is None
            if k.get("w_scales") is not None:
                assert w.dtype == torch.uint8 and k["w_scales"].dtype == torch.uint8
                self.mx += 1
            else:
                assert w.dtype == torch.bfloat16
                self.bf16 += 1
            return real(x, w, *a, **k)

        monkeypatch.setattr(llama.ops, "stream_gemm", spy)


def _prefill_meta(T, bt, bs):
    i32 = dict(dtype=torch.int32, device=DEV)
    return AttnMeta(decode=False, positions=torch.arange(T, **i32), slots=bt[0, 0].long() * bs + torch.arange(T, device=DEV),
                    block_tables=bt, ctx_lens=torch.tensor([T], **i32), cu_q=torch.tensor([0, T], **i32), max_q=T)


def _decode(model, B, seed):
    """Prefill B short prompts but their last token, then one decode step: (hidden, logits, K cache)."""
    bs, nbp = 64, 2
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(50, 100, (B,), generator=g).tolist()  # (>= 3 x 49 prefill tokens: a GEMM step)
    prompts = [torch.randint(0, TOY.vocab_size, (n,), generator=g).tolist() for n in lens]
    kv = KVCache(TOY.layers, B * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
    bt = torch.arange(B * nbp, **i32).view(B, nbp)
    # one packed prefill of every prompt's head (a GEMM step: the same bf16 copy in both models)
    ids = torch.tensor([t for p in prompts for t in p[:-1]], **i32)
    pos = torch.cat([torch.arange(len(p) - 1, **i32) for p in prompts])
    slots = torch.cat([bt[b, 0].long() * bs + torch.arange(len(p) - 1, device=DEV) for b, p in enumerate(prompts)])
    cu = torch.tensor([0] + torch.tensor([len(p) - 1 for p in prompts]).cumsum(0).tolist(), **i32)
    model.forward(ids, AttnMeta(decode=False, positions=pos, slots=slots, block_tables=bt,
                                ctx_lens=torch.tensor([len(p) - 1 for p in prompts], **i32), cu_q=cu,
                                max_q=max(lens) - 1), kv)
    dpos = torch.tensor([len(p) - 1 for p in prompts], **i32)
    ws = ops.DecodeWorkspace(B, TOY.heads, TOY.head_dim, nbp * bs // 512 + 1, DEV)
    meta = AttnMeta(decode=True, positions=dpos, slots=bt[:, 0].long() * bs + dpos.long(), block_tables=bt,
                    ctx_lens=dpos + 1, workspace=ws)
    h = model.forward(torch.tensor([p[-1] for p in prompts], **i32), meta, kv)
    return h, model.logits(h), kv.k


@pytest.mark.parametrize("B", [3, 40, 100, 130])
def test_model_decode_step_is_bit_equal(B, toy_models, monkeypatch):
    m4, m16 = toy_models
    cfgs = _streams(m4, B)
    nat = ops.native()
    assert cfgs == _streams(m16, B)
    # precondition: the projections stream, on configurations with an MXFP4 arm (at 129..256 rows
    # gate_up runs the mid-M GEMM by the model's dispatch -- on the bf16 copy of the same values)
    streamed = [n for n in PROJ if not (B > 128 and n == "gate_up_w")]
    assert all(cfgs[n] >= 0 and nat.stream_gemm_mxfp4_ok(cfgs[n]) for n in streamed), cfgs
    if B > 128:
        assert all(cfgs[n] == 27 for n in streamed), cfgs
    want_mx, want_bf16 = TOY.layers * len(streamed), 1  # (+ the bf16 LM head)
    if 64 < B <= 128:
        assert cfgs["gate_up_w"] == LlamaModel.STREAM_WIDE["gate_up"]
    calls = _Calls(monkeypatch)
    got = _decode(m4, B, B)
    assert (calls.mx, calls.bf16) == (want_mx, want_bf16)
    calls.mx = calls.bf16 = 0
    want = _decode(m16, B, B)
    assert calls.mx == 0 and calls.bf16 == TOY.layers * len(streamed) + 1
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert bool(got[0].float().abs().sum() > 0)


def test_stream_off_switches_fall_back_to_the_bf16_copy(toy_models, monkeypatch):
    """``MXFP4_STREAM_OFF`` (per projection and cfg) and ``mxfp4_stream`` stream the bf16 copy: the same bits."""
    m4, _ = toy_models
    B = 40
    cfgs = _streams(m4, B)
    calls = _Calls(monkeypatch)
    base = _decode(m4, B, B)
    assert calls.mx == TOY.layers * 4
    calls.mx = calls.bf16 = 0
    monkeypatch.setattr(m4, "MXFP4_STREAM_OFF", frozenset({("down", cfgs["down_w"]), ("qkv", 99)}))
    off = _decode(m4, B, B)
    assert (calls.mx, calls.bf16) == (TOY.layers * 3, TOY.layers + 1)
    calls.mx = calls.bf16 = 0
    monkeypatch.setattr(m4, "mxfp4_stream", False)
    none = _decode(m4, B, B)
    assert (calls.mx, calls.bf16) == (0, TOY.layers * 4 + 1)
    for a, b, c in zip(base, off, none):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_model_small_batch_fused_norm_path_is_bit_equal(monkeypatch):
    """``_layer_small`` (consumer RMSNorm, residual producers on cfg 32) on the MXFP4 copies."""
    w = _toy_weights(8)
    m4 = LlamaModel(TOY, dict(w), DEV, interleaved_mlp=True, weight_dtype="mxfp4", small_norm_fused=True)
    m16 = LlamaModel(TOY, _dequantised(w), DEV, interleaved_mlp=True, small_norm_fused=True)
    calls = _Calls(monkeypatch)
    got = _decode(m4, 5, 1)
    assert calls.mx == TOY.layers * 4
    want = _decode(m16, 5, 1)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    m4.set_proj_group("qkv", 8)  # re-lays both copies in place
    m4.set_proj_group("gate_up", 1)
    assert m4.layers[0].qkv_w.group == 8 and m4.layers[0].gate_up_w.group == 1
    again = _decode(m4, 5, 1)
    for a, b in zip(again, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("T", [64, 300])
def test_model_prefill_is_bit_equal(T, toy_models, monkeypatch):
    """64 tokens: the streamed short-prefill path (MXFP4 copies); 300: the MFMA GEMMs (bf16 copies)."""
    m4, m16 = toy_models
    bs = 64
    nb = -(-T // bs)
    ids = torch.randint(0, TOY.vocab_size, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(DEV)
    bt = torch.arange(nb, dtype=torch.int32, device=DEV).view(1, nb)
    calls = _Calls(monkeypatch)
    out = []
    for m in (m4, m16):
        kv = KVCache(TOY.layers, nb, TOY.kv_heads, bs, TOY.head_dim, DEV)
        out.append((m.forward(ids, _prefill_meta(T, bt, bs), kv), kv.k, kv.v))
    if T <= LlamaModel.PREFILL_STREAM_MAX_M:
        cfgs = _streams(m4, T)
        assert all(c >= 0 and ops.native().stream_gemm_mxfp4_ok(c) for c in cfgs.values()), cfgs
        assert calls.mx == TOY.layers * 4 and calls.bf16 == TOY.layers * 4
    else:
        assert calls.mx == 0 and calls.bf16 == 0
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_model_refusals():
    with pytest.raises(ValueError, match="tensor parallelism"):
        LlamaModel(TOY, {}, DEV, weight_dtype="mxfp4", tp_size=2, tp_rank=0)
    with pytest.raises(ValueError, match="fp8_weights_only"):
        LlamaModel(TOY, {}, DEV, weight_dtype="mxfp4", fp8_weights_only=True)


# ------------------------------------------------------------------------------------------------- engine


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_greedy_tokens_equal_the_dequantised_engine(kv_dtype, monkeypatch):
    from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams

    w = _toy_weights(4)
    prompts = [list(range(10, 10 + n)) for n in (10, 77, 150, 300)]
    greedy = SamplingParams(max_new_tokens=24, do_sample=False, temperature=0.0, ignore_eos=True)
    calls = _Calls(monkeypatch)
    outs = {}
    numel = sum(v.numel() for k, v in w.items() if k.endswith(PROJ))
    for name, weights, wd, graphs in (("mx_graphs", w, "mxfp4", True), ("mx_eager", w, "mxfp4", False),
                                      ("dequantised", _dequantised(w), None, True)):
        eng = LLMEngine(TOY, device=DEV, weights=dict(weights), max_batch=8, block_size=64, num_blocks=64,
                        max_prefill_tokens=256, max_model_len=384, use_graphs=graphs, weight_dtype=wd,
                        kv_cache_dtype=kv_dtype)
        assert eng.weight_dtype == (wd or "bf16") and eng.stats["weight_bits"] == (4 if wd else 16)
        assert eng.stats["kv_cache_bits"] == (8 if kv_dtype == "fp8" else 16)
        assert eng.stats["weight_bytes"] == (numel * 2 + numel // 2 + numel // 32 if wd else numel * 2)
        calls.mx = 0
        rids = [eng.add_request(p, greedy) for p in prompts]
        while eng.has_unfinished():
            eng.step()
        outs[name] = [eng.pop_output(r).token_ids for r in rids]
        assert (eng.stats["graph_replays"] > 0) == graphs
        assert (calls.mx > 0) == (wd == "mxfp4")
    assert all(len(t) == 24 for t in outs["mx_graphs"])
    assert outs["mx_graphs"] == outs["mx_eager"] == outs["dequantised"]
