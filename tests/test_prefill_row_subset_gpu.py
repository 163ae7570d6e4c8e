"""Row-subset prefill tail on the GPU: ``gemm_bt(..., rows=r)`` / ``gemm256(..., rows=r)`` equal the
rows of the full call bit for bit and touch nothing else; ``LlamaModel.forward(..., out_rows=sel)``
equals ``forward(...)[sel]`` with the same KV cache; the engine generates the same tokens with the
pruned path on and off."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams
from django_assistant_bot_amd.models.configs import decoder_config
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel
from django_assistant_bot_amd.models.weights import random_decoder_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
M = 1300  # five row tiles of 256, the last one ragged (20 rows)
CANARY = -7.0
GUARD = 3  # canary rows before and after a guarded view

ROWS = {
    "tile-edges-unsorted": [0, 255, 256, 1299, 7],
    "one-row": [777],
    "more-than-a-tile": [(37 * i + 5) % M for i in range(257)],  # 257 rows: two row tiles of the compact C
    "duplicates": [1024, 3, 1024, 1299, 3, 1024],
}


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF).to(DEV)


def _guarded(n, cols):
    """(buffer, view [n, cols]) inside canary rows and canary columns."""
    buf = torch.full((n + 2 * GUARD, cols + 16), CANARY, dtype=BF, device=DEV)
    return buf, buf[GUARD:GUARD + n, :cols]


def _only_view_written(buf, n, cols):
    b = buf.clone()
    b[GUARD:GUARD + n, :cols] = CANARY
    return bool((b == CANARY).all())


_FULL: dict = {}


def _case(variant, K):
    """Operands and the full call's output of one (variant, K), computed once and left unchanged."""
    key = (variant, K)
    if key not in _FULL:
        A = _rand((M, K), 1 + K, 0.5)
        if variant == "swiglu8":
            # at N = 1024 the dispatcher gives the full M = 1300 call to gemm_mid, so this variant calls
            # the 256 x 256 kernel itself on both sides
            W = ops.shuffle_weights(_rand((1024, K), 2 + K, 0.2), 8)
            kw = dict(epilogue=ops.EPI_SWIGLU8, shuffled=True, b_group=8)
            R, fn = None, ops.kernels.gemm256
        else:
            W = _rand((512, K), 3 + K, 0.2)
            R = _rand((M, 512), 4 + K) if variant == "residual" else None
            kw, fn = {}, ops.gemm_bt
        full = fn(A, W, residual=R, **kw)
        torch.cuda.synchronize()
        _FULL[key] = (A, W, R, kw, fn, full)
    return _FULL[key]


@pytest.mark.parametrize("K", [256, 4096])
@pytest.mark.parametrize("variant", ["plain", "residual", "swiglu8"])
@pytest.mark.parametrize("rows", sorted(ROWS))
def test_rows_equal_the_full_calls_rows(rows, variant, K):
    A, W, R, kw, fn, full = _case(variant, K)
    a0, r0 = A.clone(), None if R is None else R.clone()
    r = torch.tensor(ROWS[rows], dtype=torch.int32, device=DEV)
    n, n_out = r.numel(), full.shape[1]
    buf, view = _guarded(n, n_out)
    got = fn(A, W, residual=R, rows=r, out=view, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr()
    assert torch.equal(view, full[r.long()])
    assert _only_view_written(buf, n, n_out)
    assert torch.equal(A, a0) and (R is None or torch.equal(R, r0))
    assert torch.equal(fn(A, W, residual=R, rows=r, **kw), full[r.long()])  # an output of its own


def test_rows_follow_the_dispatch_on_a_grouped_shuffled_copy():
    """gate_up-like shape whose full call the dispatcher gives to gemm256 (6 x 32 = 192 tiles): SwiGLU8
    over a ``shuffle_weights(w, 8)`` copy through ``gemm_bt``, ``rows`` and ``as_m``."""
    K, N = 256, 8192
    A, W = _rand((M, K), 11, 0.5), ops.shuffle_weights(_rand((N, K), 12, 0.2), 8)
    kw = dict(epilogue=ops.EPI_SWIGLU8, shuffled=True, b_group=8)
    assert not ops.kernels.use_gemm_mid(M, N, K, K) and ops.kernels.use_gemm256(M, N, K, K, K)
    full = ops.gemm_bt(A, W, **kw)
    r = torch.tensor(ROWS["tile-edges-unsorted"], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.gemm_bt(A, W, rows=r, **kw), full[r.long()])
    compact = A[r.long()].contiguous()
    assert torch.equal(ops.gemm_bt(compact, W, as_m=M, **kw), full[r.long()])
    assert ops.gemm_bt(A, W, rows=r[:0], **kw).shape == (0, N // 2)


def test_rows_are_refused_where_the_full_call_is_not_gemm256():
    r = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    K = 256
    A = _rand((M, K), 21)
    Wm = ops.shuffle_weights(_rand((512, K), 22))
    assert ops.kernels.use_gemm_mid(M, 512, K, K)  # 12 tiles: the stream-K kernel
    with pytest.raises(ValueError):
        ops.gemm_bt(A, Wm, shuffled=True, rows=r)
    with pytest.raises(ValueError):
        ops.gemm_bt(A[:2].contiguous(), Wm, shuffled=True, as_m=M)
    W = _rand((512, K), 23)
    assert not ops.kernels.use_gemm256(300, 512, K, K, K)  # the 128 x 128 kernel
    with pytest.raises(ValueError):
        ops.gemm_bt(A[:300], W, rows=r)
    with pytest.raises(ValueError):
        ops.gemm_bt(A, W, bias=_rand((512,), 24), rows=r)


# ------------------------------------------------------------------------------------------------
# model: 2 layers at Llama-3-8B width


@pytest.fixture(scope="module")
def model8b():
    cfg = decoder_config("llama-3-8b", layers=2)
    w = random_decoder_weights(cfg, device=DEV, dtype=BF, seed=3, interleave_mlp=True)
    for i in range(cfg.layers):  # non-unit norm gains
        for n in ("attn_norm", "mlp_norm"):
            w[f"l{i}.{n}"] = (0.5 + torch.rand(cfg.hidden, generator=torch.Generator().manual_seed(i))).to(BF).to(DEV)
    m = LlamaModel(cfg, w, DEV, interleaved_mlp=True, consume=True)
    assert m.frag
    return cfg, m


def _packed(cfg, lens, seed=0):
    bs = 64
    i32 = dict(dtype=torch.int32, device=DEV)
    nblk = [-(-n // bs) for n in lens]
    bt = torch.zeros((len(lens), max(nblk)), **i32)
    o = 0
    for b, nb in enumerate(nblk):
        bt[b, :nb] = torch.arange(o, o + nb, **i32)
        o += nb
    pos = torch.cat([torch.arange(n, **i32) for n in lens])
    slots = torch.cat([(bt[b, torch.arange(n, device=DEV) // bs].long() * bs + torch.arange(n, device=DEV) % bs)
                       for b, n in enumerate(lens)])
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), **i32)
    ids = torch.randint(0, 128000, (sum(lens),), generator=torch.Generator().manual_seed(seed)).to(**i32)
    meta = AttnMeta(decode=False, positions=pos, slots=slots, block_tables=bt, ctx_lens=torch.tensor(lens, **i32),
                    cu_q=cu, max_q=max(lens))
    return ids, meta, lambda: KVCache(cfg.layers, sum(nblk), cfg.kv_heads, bs, cfg.head_dim, DEV)


def _count_calls(monkeypatch):
    """Row-subset GEMM launches (``gemm_bt`` calls with ``rows`` or ``as_m``)."""
    calls = []
    orig = ops.gemm_bt

    def spy(*a, **k):
        if k.get("rows") is not None or k.get("as_m") is not None:
            calls.append(1)
        return orig(*a, **k)

    monkeypatch.setattr(ops, "gemm_bt", spy)
    return calls


def _mid_off(monkeypatch):
    """At Llama-3-8B width the dispatcher keeps o / down (N = 4096) on gemm_mid below T = 2817 (192
    tiles); the T = 1280 cases run on the gemm256 path, the full reference included, by switching
    the stream-K kernel off.  ``test_forward_prunes_under_the_real_dispatch`` needs no switch."""
    monkeypatch.setattr(ops.kernels, "GEMM_MID_MIN_M", 1 << 30)


@pytest.fixture(scope="module")
def full1280(model8b):
    cfg, m = model8b
    lens = [700, 333, 247]
    assert sum(lens) == 1280
    ids, meta, new_kv = _packed(cfg, lens)
    kv = new_kv()
    with pytest.MonkeyPatch.context() as mp:
        _mid_off(mp)
        h = m.forward(ids, meta, kv)
    torch.cuda.synchronize()
    return lens, ids, meta, new_kv, kv, h


@pytest.mark.parametrize("sel", ["last-rows", "mid-prompt", "empty"])
def test_forward_out_rows_equals_the_full_forwards_rows(model8b, full1280, sel, monkeypatch):
    cfg, m = model8b
    lens, ids, meta, new_kv, kv_full, h_full = full1280
    _mid_off(monkeypatch)
    rows = {"last-rows": [699, 1032, 1279], "mid-prompt": [850], "empty": []}[sel]
    r = torch.tensor(rows, dtype=torch.int32, device=DEV)
    calls = _count_calls(monkeypatch)
    kv = new_kv()
    h = m.forward(ids, meta, kv, out_rows=r)
    torch.cuda.synchronize()
    assert h.shape == (len(rows), cfg.hidden)
    assert torch.equal(h, h_full[r.long()])
    assert torch.equal(kv.k, kv_full.k) and torch.equal(kv.v, kv_full.v)
    assert len(calls) == (3 if rows else 0)  # o, gate_up, down of the last layer only (none for no rows)
    # int64 row ids (what index_select took before) are accepted too
    if rows:
        assert torch.equal(m.forward(ids, meta, new_kv(), out_rows=r.long()), h)


def test_forward_prunes_under_the_real_dispatch(model8b, monkeypatch):
    """T = 2880: 12 row tiles x 16 = 192 tiles, the first size at which o and down run on gemm256."""
    cfg, m = model8b
    lens = [1500, 900, 480]
    ids, meta, new_kv = _packed(cfg, lens, seed=2)
    kv_full, kv = new_kv(), new_kv()
    h_full = m.forward(ids, meta, kv_full)
    r = torch.tensor([1499, 2399, 2879], dtype=torch.int32, device=DEV)
    calls = _count_calls(monkeypatch)
    h = m.forward(ids, meta, kv, out_rows=r)
    torch.cuda.synchronize()
    assert len(calls) == 3
    assert torch.equal(h, h_full[r.long()])
    assert torch.equal(kv.k, kv_full.k) and torch.equal(kv.v, kv_full.v)


def test_forward_out_rows_keeps_the_old_path_at_mid_m(model8b, monkeypatch):
    cfg, m = model8b
    lens = [150, 90, 60]  # T = 300: gemm_mid
    ids, meta, new_kv = _packed(cfg, lens, seed=1)
    kv_full, kv = new_kv(), new_kv()
    h_full = m.forward(ids, meta, kv_full)
    assert h_full.shape == (300, cfg.hidden)
    r = torch.tensor([149, 239, 299], dtype=torch.int32, device=DEV)
    calls = _count_calls(monkeypatch)
    h = m.forward(ids, meta, kv, out_rows=r)
    torch.cuda.synchronize()
    assert not calls
    assert torch.equal(h, h_full[r.long()])
    assert torch.equal(kv.k, kv_full.k) and torch.equal(kv.v, kv_full.v)


def test_switch_off_runs_the_full_path(model8b, full1280, monkeypatch):
    cfg, m = model8b
    lens, ids, meta, new_kv, kv_full, h_full = full1280
    r = torch.tensor([699, 1032, 1279], dtype=torch.int32, device=DEV)
    _mid_off(monkeypatch)
    calls = _count_calls(monkeypatch)
    monkeypatch.setattr(LlamaModel, "prune_last_tail", False)
    assert torch.equal(m.forward(ids, meta, new_kv(), out_rows=r), h_full[r.long()])
    assert not calls


# ------------------------------------------------------------------------------------------------
# engine


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_tokens_equal_with_the_path_on_and_off(model8b, graphs, monkeypatch):
    cfg, m = model8b
    gen = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, 128000, (n,), generator=gen).tolist() for n in (1400, 900, 400, 200)]  # 2900 tokens
    greedy = SamplingParams(max_new_tokens=8, do_sample=False, temperature=0.0, ignore_eos=True)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(LlamaModel, "prune_last_tail", on)
        calls = _count_calls(monkeypatch)
        eng = LLMEngine(cfg, DEV, shared_model=m, max_batch=8, max_model_len=2048, num_blocks=64, use_graphs=graphs,
                        max_prefill_tokens=4096)
        out[on] = [o.token_ids for o in eng.generate(prompts, greedy)]
        monkeypatch.setattr(ops, "gemm_bt", ops.kernels.gemm_bt)
        assert bool(calls) == on  # the prompts fill one gemm256-sized prefill step
        assert all(len(t) == 8 for t in out[on])
    assert out[True] == out[False]
