"""MXFP4 as the only weight copy (``mxfp4_weights_only``) on the GPU: the in-launch dequantiser
``ops.weight_dequant_mxfp4`` and the one-copy ``LlamaModel`` / ``LLMEngine``.

The dequantiser writes the bf16 fragment image the two-copy model keeps resident, and every kernel then
runs unchanged on it, so nothing here is a tolerance: every comparison is ``torch.equal`` -- the image
against ``shuffle_weights(weight_dequantize_mxfp4(...))``, the one-copy model against the two-copy model
in every step kind, the engines' greedy tokens against each other."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.models.configs import DecoderConfig
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel, Mxfp4Proj
from django_assistant_bot_amd.models.weights import random_decoder_weights
from django_assistant_bot_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE_BYTES = (2, 3, 126, 127, 128, 251, 252)  # both ends of the range whose products stay normal, and 2^-1 .. 2^1
PROJ = ("qkv_w", "o_w", "gate_up_w", "down_w")
PAD = 2048  # bf16 elements = 4 KB behind the image
SENTINEL = -7.0
SHAPES = [(16, 128, 1), (16, 384, 1), (48, 256, 1), (128, 384, 8), (256, 128, 8)]


def _raw(N, K, seed):
    """Row-major codes [N, K/2] over all 16 values and scale bytes [N, K/32] drawn from SCALE_BYTES."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scales = torch.tensor(SCALE_BYTES, dtype=torch.uint8)[torch.randint(0, len(SCALE_BYTES), (N, K // 32), generator=g)]
    return codes, scales


def _dequant(codes, scales, group, grid_cap=0):
    """The kernel on row-major (codes, scales): (whole padded buffer on the CPU, N K)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    out = torch.full((N * K + PAD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    view = ops.weight_dequant_mxfp4(ops.shuffle_weights_mxfp4(codes, group).to(DEV), ops.shuffle_scales_mxfp4(scales).to(DEV),
                                    out, group, grid_cap=grid_cap)
    assert view.shape == (N, K) and view.data_ptr() == out.data_ptr()
    return out.cpu(), N * K


# ------------------------------------------------------------------------------------------- dequantiser


@pytest.mark.parametrize("N,K,group", SHAPES)
def test_dequantiser_equals_the_reference_image(N, K, group):
    codes, scales = _raw(N, K, 7 * N + K)
    assert set((codes & 15).flatten().tolist()) == set(range(16)) and set(scales.flatten().tolist()) <= set(SCALE_BYTES)
    want = ops.shuffle_weights(ops.weight_dequantize_mxfp4(codes, scales), group)
    assert bool(torch.isfinite(want.float()).all())
    out, n = _dequant(codes, scales, group)
    assert torch.equal(out[:n].view(N, K), want)
    assert bool((out[n:] == SENTINEL).all())  # nothing past N K elements


@pytest.mark.parametrize("group", [1, 8])
def test_every_code_under_every_scale_byte_at_known_positions(group):
    """One non-zero code per (code, scale byte) pair, each in an MX block of its own at a written-down
    (row, k); everything else is code 0 under scale byte 127.  The row-major image must hold exactly
    code x 2^(byte - 127) there and zero elsewhere: pins the lane / byte / chunk / scale-row map without
    the reference dequantiser."""
    N, K = 128, 384
    lut = torch.tensor(ref.MXFP4_GRID + tuple(-v for v in ref.MXFP4_GRID), dtype=torch.float64)
    codes = torch.zeros((N, K // 2), dtype=torch.uint8)
    scales = torch.full((N, K // 32), 127, dtype=torch.uint8)
    want = torch.zeros((N, K), dtype=torch.float64)
    where, kins = set(), set()
    for p, (c, s) in enumerate((c, s) for c in range(16) for s in SCALE_BYTES):
        row, blk, kin = (7 * p + 3) % N, (5 * p + 1) % (K // 32), (3 * p + p // 8) % 32
        k = 32 * blk + kin
        assert (row, blk) not in where
        where.add((row, blk))
        kins.add(kin)
        codes[row, k // 2] |= c << (4 * (k & 1))
        scales[row, blk] = s
        want[row, k] = lut[c] * 2.0 ** (s - 127)
    assert {b for _, b in where} == set(range(K // 32))  # every chunk of every 128-deep fragment
    assert len({r // 16 for r, _ in where}) == N // 16  # every 16-row block
    assert kins == set(range(32))  # every lane quadrant, every byte of a lane's dword, both nibbles
    out, n = _dequant(codes, scales, group)
    got = ops.unshuffle_weights(out[:n].view(N, K), group)
    assert torch.equal(got.double(), want)  # (every product is a bf16)
    assert int((got != 0).sum()) == 14 * len(SCALE_BYTES)  # (codes 0 and 8 are zeros)
    assert bool((out[n:] == SENTINEL).all())


def test_grid_stride_loop_gives_the_same_bytes():
    N, K, group = 128, 384, 8  # 1536 lanes: 6 workgroups by default
    codes, scales = _raw(N, K, 11)
    base, n = _dequant(codes, scales, group)
    assert torch.equal(base[:n].view(N, K), ops.shuffle_weights(ops.weight_dequantize_mxfp4(codes, scales), group))
    for cap in (1, 3):
        out, _ = _dequant(codes, scales, group, grid_cap=cap)
        assert torch.equal(out.view(torch.int16), base.view(torch.int16)), cap


def test_non_temporal_store_arm_gives_the_same_bytes():
    nat = ops.native()
    codes, scales = _raw(128, 384, 12)
    old = nat.weight_dequant_mxfp4_nt()
    try:
        nat.weight_dequant_mxfp4_set_nt(0)
        a, _ = _dequant(codes, scales, 8)
        nat.weight_dequant_mxfp4_set_nt(1)
        assert nat.weight_dequant_mxfp4_nt() == 1
        b, _ = _dequant(codes, scales, 8, grid_cap=2)
    finally:
        nat.weight_dequant_mxfp4_set_nt(old)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_invalid_launches_raise_and_leave_out_untouched(monkeypatch):
    nat = ops.native()
    N, K = 128, 256
    codes, scales = _raw(N, K, 13)
    c4, sc = ops.shuffle_weights_mxfp4(codes).to(DEV), ops.shuffle_scales_mxfp4(scales).to(DEV)
    out = torch.full((N * K + PAD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    launched = []
    real = nat.weight_dequant_mxfp4
    monkeypatch.setattr(nat, "weight_dequant_mxfp4", lambda *a, **k: launched.append(1) or real(*a, **k))
    off16 = torch.empty(c4.numel() + 16, dtype=torch.uint8, device=DEV)[8:8 + c4.numel()].view(c4.shape).copy_(c4)
    off4 = torch.empty(sc.numel() + 4, dtype=torch.uint8, device=DEV)[2:2 + sc.numel()].view(sc.shape).copy_(sc)
    bad = [
        (c4[:, :96].contiguous(), sc[:, :6].contiguous(), out, 1),  # K % 128
        (c4[:24].contiguous(), sc[:24].contiguous(), out, 1),  # N % 16
        (c4[:64].contiguous(), sc[:64].contiguous(), out, 8),  # N % (16 group)
        (c4.to(torch.int8), sc, out, 1), (c4, sc.to(torch.int32), out, 1), (c4, sc, out.float(), 1),  # dtypes
        (c4, sc, out.view(torch.float16), 1),
        (off16, sc, out, 1), (c4, off4, out, 1), (c4, sc, out[4:], 1),  # misaligned views
        (c4, sc, out[:N * K - 8], 1), (c4, sc[:-16], out, 1), (c4, sc, out.cpu(), 1),
    ]
    for c, s, o, g in bad:
        with pytest.raises(ValueError):
            ops.weight_dequant_mxfp4(c, s, o, g)
    assert launched == []
    monkeypatch.undo()
    # the entry point itself: hipErrorInvalidValue before any launch
    st = torch.cuda.current_stream().cuda_stream

    def raw(codes_=c4.data_ptr(), scales_=sc.data_ptr(), out_=out.data_ptr(), N_=N, K_=K, group=1, cap=0):
        nat.weight_dequant_mxfp4(codes_, scales_, out_, N_, K_, group, cap, st)

    for kw in (dict(K_=K + 64), dict(K_=0), dict(N_=N + 8), dict(N_=64, group=8), dict(group=0), dict(cap=-1),
               dict(codes_=0), dict(scales_=0), dict(out_=0), dict(codes_=c4.data_ptr() + 8),
               dict(scales_=sc.data_ptr() + 2), dict(out_=out.data_ptr() + 8),
               dict(N_=1 << 15, K_=1 << 15, group=8)):  # N K 2 = 2^31 bytes with a grouped layout
        with pytest.raises(RuntimeError, match="weight_dequant_mxfp4"):
            raw(**kw)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    raw()
    assert torch.equal(out[:N * K].view(N, K).cpu(), ops.shuffle_weights(ops.weight_dequantize_mxfp4(codes, scales)))
    assert bool((out[N * K:] == SENTINEL).all())


# -------------------------------------------------------------------------------------------------- model

# the toy decoder of tests/test_weight_mxfp4_gpu.py: qkv [1024, 512], o [512, 512], gate_up [1792, 512],
# down [512, 896]; every N % 256 == 0 and K % 128 == 0
TOY = DecoderConfig("toy-w4", vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, intermediate=896,
                    max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)
NATIVE_GEMMS = ("gemm_bt", "gemm256", "gemm_mid", "stream_gemm", "stream_gemm_mxfp4")


def _toy_weights(seed):
    return {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(TOY, dtype=torch.float32, seed=seed,
                                                                       interleave_mlp=True).items()}


def _numels(model_or_weights):
    if isinstance(model_or_weights, dict):
        return [v.numel() for k, v in model_or_weights.items() if k.endswith(PROJ)]
    return [getattr(L, n).shape[0] * getattr(L, n).shape[1] for L in model_or_weights.layers for n in PROJ]


@pytest.fixture(scope="module")
def toy_models():
    """(one-copy model, two-copy model) from the same weights, with the bytes each allocated."""
    w = _toy_weights(6)
    torch.cuda.synchronize()
    alloc = []
    models = []

    def held():
        # the bytes the live tensors asked for: ``memory_allocated`` also counts what the caching allocator
        # rounds up (a request served from a cached block up to 1 MB larger keeps the whole block)
        return torch.cuda.memory_stats()["requested_bytes.all.current"]

    for only in (False, True):
        before = held()
        models.append(LlamaModel(TOY, dict(w), DEV, interleaved_mlp=True, weight_dtype="mxfp4", mxfp4_weights_only=only))
        alloc.append(held() - before)
    m2, m1 = models
    numels = _numels(w)
    assert m1.frag and m1.mxfp4_weights_only and not m2.mxfp4_weights_only and m1.proj_group == m2.proj_group
    assert m1.proj_group["gate_up"] == 8
    for L1, L2 in zip(m1.layers, m2.layers):
        for n in PROJ:
            p1, p2 = getattr(L1, n), getattr(L2, n)
            assert isinstance(p1, Mxfp4Proj) and isinstance(p2, Mxfp4Proj) and p1.w is None and p2.w is not None
            assert tuple(p1.shape) == tuple(p2.shape) == tuple(p2.w.shape) and p1.group == p2.group
            assert torch.equal(p1.data, p2.data) and torch.equal(p1.scales, p2.scales)
    assert m1.projection_bytes() == sum(n // 2 + n // 32 for n in numels)
    assert m2.projection_bytes() == m1.projection_bytes() + sum(2 * n for n in numels)
    assert m1.mxfp4_scratch_bytes() == 2 * max(numels) and m2.mxfp4_scratch_bytes() == 0
    assert alloc[1] <= alloc[0] - sum(2 * n for n in numels) + m1.mxfp4_scratch_bytes(), alloc
    return m1, m2


class _Spy:
    """Counts the native GEMM entry points and the dequantiser by name."""

    def __init__(self, monkeypatch):
        self.n = {}
        self.outs = []  # the dequantiser's output pointers
        nat = ops.native()
        for name in NATIVE_GEMMS + ("weight_dequant_mxfp4",):
            monkeypatch.setattr(nat, name, self._wrap(name, getattr(nat, name)))

    def _wrap(self, name, real):
        def f(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            if name == "weight_dequant_mxfp4":
                self.outs.append(a[2])
            return real(*a, **k)
        return f

    def take(self):
        n, self.n = self.n, {}
        return n


def _prefill_meta(lens, bt, bs):
    """Packed prefill of len(lens) fresh sequences, sequence i in the blocks of row i of ``bt``."""
    i32 = dict(dtype=torch.int32, device=DEV)
    pos = torch.cat([torch.arange(n, **i32) for n in lens])
    slots = torch.cat([bt[i, 0].long() * bs + torch.arange(n, device=DEV) for i, n in enumerate(lens)])
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), **i32)
    return AttnMeta(decode=False, positions=pos, slots=slots, block_tables=bt, ctx_lens=torch.tensor(lens, **i32),
                    cu_q=cu, max_q=max(lens))


def _prefill(model, lens, out_rows=None):
    bs = 64
    nbp = -(-max(lens) // bs)
    T = sum(lens)
    ids = torch.randint(0, TOY.vocab_size, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(DEV)
    bt = torch.arange(len(lens) * nbp, dtype=torch.int32, device=DEV).view(len(lens), nbp)
    kv = KVCache(TOY.layers, len(lens) * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
    rows = None if out_rows is None else torch.tensor(out_rows, dtype=torch.int32, device=DEV)
    return model.forward(ids, _prefill_meta(lens, bt, bs), kv, out_rows=rows), kv.k, kv.v


def _decode(model, B, seed, spy=None):
    """Prefill B short prompts but their last token, then one decode step: (hidden, logits, K, V);
    the spy's counts are those of the decode step alone."""
    bs, nbp = 64, 1
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(20, 60, (B,), generator=g).tolist()
    prompts = [torch.randint(0, TOY.vocab_size, (n,), generator=g).tolist() for n in lens]
    kv = KVCache(TOY.layers, B * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
    bt = torch.arange(B * nbp, **i32).view(B, nbp)
    ids = torch.tensor([t for p in prompts for t in p[:-1]], **i32)
    model.forward(ids, _prefill_meta([n - 1 for n in lens], bt, bs), kv)
    if spy is not None:
        spy.take()
    dpos = torch.tensor([n - 1 for n in lens], **i32)
    ws = ops.DecodeWorkspace(B, TOY.heads, TOY.head_dim, nbp * bs // 512 + 1, DEV)
    meta = AttnMeta(decode=True, positions=dpos, slots=bt[:, 0].long() * bs + dpos.long(), block_tables=bt,
                    ctx_lens=dpos + 1, workspace=ws)
    h = model.forward(torch.tensor([p[-1] for p in prompts], **i32), meta, kv)
    return h, model.logits(h), kv.k, kv.v


def _mixed(model):
    bs, nbp = 64, 4
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(2)
    dec = [torch.randint(0, 900, (n,), generator=g).tolist() for n in (40, 130, 77)]
    pre = [torch.randint(0, 900, (n,), generator=g).tolist() for n in (90, 33)]
    nd, npf = len(dec), len(pre)
    dbt = torch.arange(nd * nbp, **i32).view(nd, nbp)
    dpos = torch.tensor([len(p) - 1 for p in dec], **i32)
    pbt = torch.arange(nd * nbp, (nd + npf) * nbp, **i32).view(npf, nbp)
    ids = torch.tensor([t for p in pre for t in p] + [p[-1] for p in dec], **i32)
    pos = torch.cat([torch.arange(len(p), **i32) for p in pre] + [dpos])
    slots = torch.cat([pbt[i, 0].long() * bs + torch.arange(len(p), device=DEV) for i, p in enumerate(pre)]
                      + [dbt[:, 0].long() * bs + dpos.long()])
    kv = KVCache(TOY.layers, (nd + npf) * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
    for b, p in enumerate(dec):
        model.forward(torch.tensor(p[:-1], **i32), _prefill_meta([len(p) - 1], dbt[b:b + 1], bs), kv)
    ws = ops.DecodeWorkspace(8, TOY.heads, TOY.head_dim, nbp * bs // 512 + 1, DEV)
    meta = AttnMeta(decode=False, positions=pos, slots=slots, block_tables=pbt,
                    ctx_lens=torch.tensor([len(p) for p in pre], **i32),
                    cu_q=torch.tensor([0, len(pre[0]), len(pre[0]) + len(pre[1])], **i32), max_q=90, workspace=ws,
                    n_decode=nd, dec_block_tables=dbt, dec_ctx_lens=dpos + 1)
    return model.forward(ids, meta, kv), kv.k, kv.v


def _both(models, spy, fn):
    """fn(model) on the one-copy and the two-copy model: asserts equal tensors, the same GEMM launches and
    one dequantiser launch per launch that read a bf16 projection; -> the one-copy model's counts."""
    m1, m2 = models
    got = fn(m1)
    n1 = spy.take()
    want = fn(m2)
    n2 = spy.take()
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)
    assert bool(got[0].float().abs().sum() > 0)
    assert n2.pop("weight_dequant_mxfp4", 0) == 0
    deq = n1.pop("weight_dequant_mxfp4", 0)
    assert n1 == n2, (n1, n2)  # dispatch is unchanged
    return n1, deq


def _bf16_launches(n, lm_head=0):
    return sum(v for k, v in n.items() if k != "stream_gemm_mxfp4") - lm_head


@pytest.mark.parametrize("B", [1, 16, 64, 128, 200])
def test_model_decode_step_is_bit_equal(B, toy_models, monkeypatch):
    spy = _Spy(monkeypatch)
    n, deq = _both(toy_models, spy, lambda m: _decode(m, B, B, spy))
    L = TOY.layers
    if B <= 128:  # every projection streams the codes; the LM head is bf16
        assert n == {"stream_gemm_mxfp4": 4 * L, "stream_gemm": 1} and deq == 0
    else:  # 129..256: gate_up on gemm_mid, through the scratch
        assert n == {"stream_gemm_mxfp4": 3 * L, "gemm_mid": L, "stream_gemm": 1} and deq == L


def _family_lens():
    """{kernel family: sequence lengths of a prefill step whose four projections all take it} on the
    two-copy model's dispatch (``ops.gemm_bt``), searched in the dispatch predicates themselves."""
    K = ops.kernels
    shapes = [(1024, 512), (512, 512), (1792, 512), (512, 896)]

    def family(T):
        if T <= LlamaModel.PREFILL_STREAM_MAX_M:
            return "stream"
        f = {("gemm_mid" if K.use_gemm_mid(T, N, Kd, Kd) else "gemm256" if K.use_gemm256(T, N, Kd, Kd, Kd) else "gemm_bt")
             for N, Kd in shapes}
        return f.pop() if len(f) == 1 else None

    out = {}
    for lens in ([64], [300], [K.GEMM256_MIN_M], [1400, 1400, 1400], [1100] * 8):
        out.setdefault(family(sum(lens)), lens)
    return out


@pytest.mark.parametrize("fam", ["stream", "gemm_mid", "gemm256"])
def test_model_prefill_is_bit_equal_per_kernel_family(fam, toy_models, monkeypatch):
    lens = _family_lens().get(fam)
    assert lens is not None, f"no prefill size of the toy decoder dispatches {fam}"
    spy = _Spy(monkeypatch)
    n, deq = _both(toy_models, spy, lambda m: _prefill(m, lens))
    L = TOY.layers
    if fam == "stream":
        assert n == {"stream_gemm_mxfp4": 4 * L} and deq == 0
    else:
        assert n == {fam: 4 * L} and deq == 4 * L


def test_model_prefill_on_the_128x128_kernel_is_bit_equal(toy_models, monkeypatch):
    """The toy's shapes (every N % 256 == 0) reach the 128 x 128 kernel at no size while gemm_mid takes
    mid-M from the first row, so gemm_mid is switched off for this step (its A/B constant): T = 300 is
    then below gemm256's range too."""
    monkeypatch.setattr(ops.kernels, "GEMM_MID_MIN_M", 1 << 30)
    spy = _Spy(monkeypatch)
    n, deq = _both(toy_models, spy, lambda m: _prefill(m, [300]))
    assert n == {"gemm_bt": 4 * TOY.layers} and deq == 4 * TOY.layers


def test_model_prefill_with_out_rows_is_bit_equal(toy_models, monkeypatch):
    """The pruned last-layer tail (a gemm256 step: o gathers its rows, gate_up / down run ``as_m``) and a
    step that runs whole and selects afterwards."""
    lens = _family_lens()["gemm256"]
    m1, m2 = toy_models
    T = sum(lens)
    x = torch.empty(1, device=DEV)
    meta = AttnMeta(decode=False, positions=x, slots=x, block_tables=x, ctx_lens=x)
    assert m1._tail_prunable(T, meta, x, False) and m2._tail_prunable(T, meta, x, False)
    rows = [lens[0] - 1, lens[0] + lens[1] - 1, T - 1, 5]
    spy = _Spy(monkeypatch)
    n, deq = _both(toy_models, spy, lambda m: _prefill(m, lens, rows))
    assert n == {"gemm256": 4 * TOY.layers} and deq == 4 * TOY.layers
    full = _prefill(m1, lens)[0]
    assert torch.equal(_prefill(m1, lens, rows)[0], full[torch.tensor(rows, device=DEV)])
    assert not m1._tail_prunable(300, meta, x, False)
    spy.take()
    n, deq = _both(toy_models, spy, lambda m: _prefill(m, [300], [299, 0, 17]))
    assert deq == 4 * TOY.layers == _bf16_launches(n)


def test_model_mixed_step_is_bit_equal(toy_models, monkeypatch):
    spy = _Spy(monkeypatch)

    def run(m):
        out = _mixed(m)
        return out

    n, deq = _both(toy_models, spy, run)
    # (the three warm-up prefills of 39 / 129 / 76 tokens and the 126-token mixed step)
    assert deq == _bf16_launches(n) > 0 and n.get("stream_gemm", 0) == 0


def test_model_with_streaming_off_reads_the_scratch_everywhere(toy_models, monkeypatch):
    """``mxfp4_stream = False``: every decode GEMM streams the bf16 image (the two-copy model: its copy)."""
    for m in toy_models:
        monkeypatch.setattr(m, "mxfp4_stream", False)
    spy = _Spy(monkeypatch)
    L = TOY.layers
    for B, want in ((40, {"stream_gemm": 4 * L + 1}), (200, {"stream_gemm": 3 * L + 1, "gemm_mid": L})):
        n, deq = _both(toy_models, spy, lambda m: _decode(m, B, B, spy))
        assert n == want and deq == 4 * L
    n, deq = _both(toy_models, spy, lambda m: _prefill(m, [64]))
    assert n == {"stream_gemm": 4 * L} and deq == 4 * L


def test_model_after_regrouping_is_bit_equal(toy_models, monkeypatch):
    m1, m2 = toy_models
    spy = _Spy(monkeypatch)
    base = _decode(m1, 200, 200), _prefill(m1, [300])
    try:
        for m in toy_models:
            m.set_proj_group("gate_up", 1)
        assert m1.layers[0].gate_up_w.group == 1 and m1.layers[0].gate_up_w.w is None
        spy.take()
        for fn in (lambda m: _decode(m, 200, 200, spy), lambda m: _prefill(m, [300])):
            _, deq = _both(toy_models, spy, fn)
            assert deq > 0
    finally:
        for m in toy_models:
            m.set_proj_group("gate_up", 8)
    assert m1.layers[0].gate_up_w.group == 8
    assert torch.equal(m1.layers[0].gate_up_w.data, m2.layers[0].gate_up_w.data)
    again = _decode(m1, 200, 200), _prefill(m1, [300])
    for a, b in zip(base, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    _both(toy_models, spy, lambda m: _decode(m, 200, 200, spy))


def test_scratches_are_per_stream_and_capture_cannot_allocate(toy_models, monkeypatch):
    m1, _ = toy_models
    p = m1.layers[0].gate_up_w
    torch.cuda.synchronize()
    base = m1._bf16_w(p)
    assert base.shape == tuple(p.shape) and base.dtype == torch.bfloat16
    assert base.data_ptr() == m1._bf16_w(m1.layers[0].o_w).data_ptr()  # one scratch for every projection
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        mine = m1._bf16_w(p)
        assert mine.data_ptr() != base.data_ptr() and mine.data_ptr() == m1._bf16_w(p).data_ptr()
        want = ops.shuffle_weights(ops.weight_dequantize_mxfp4(
            ops.unshuffle_weights_mxfp4(p.data, p.group), ops.unshuffle_scales_mxfp4(p.scales)), p.group)
        assert torch.equal(mine, want)
    s.synchronize()
    s2 = torch.cuda.Stream()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with torch.cuda.stream(s2):
        with pytest.raises(RuntimeError, match="capture"):
            m1._bf16_w(p)
    with torch.cuda.stream(s):
        assert m1._bf16_w(p).data_ptr() == mine.data_ptr()  # (a stream that has one keeps using it)
    torch.cuda.synchronize()


def test_model_refusals_on_the_gpu():
    w = _toy_weights(1)
    with pytest.raises(ValueError, match="mxfp4_weights_only needs weight_dtype='mxfp4'"):
        LlamaModel(TOY, dict(w), DEV, interleaved_mlp=True, mxfp4_weights_only=True)
    with pytest.raises(ValueError, match="fragment layout"):
        LlamaModel(TOY, dict(w), DEV, interleaved_mlp=True, weight_dtype="mxfp4", mxfp4_weights_only=True,
                   fragment_layout=False)
    with pytest.raises(ValueError, match="fragment layout"):  # (stacked gate / up rows: no fragment layout)
        LlamaModel(TOY, dict(w), DEV, interleaved_mlp=False, weight_dtype="mxfp4", mxfp4_weights_only=True)
    # a projection with K % 128 != 0 would keep no codes
    odd = DecoderConfig("toy-w4-odd", vocab_size=1024, hidden=512, layers=1, heads=4, kv_heads=2, intermediate=832,
                        max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)
    wo = {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(odd, dtype=torch.float32, seed=1,
                                                                     interleave_mlp=True).items()}
    LlamaModel(odd, dict(wo), DEV, interleaved_mlp=True, weight_dtype="mxfp4")  # (the two-copy mode takes it)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="K % 128"):
        LlamaModel(odd, dict(wo), DEV, interleaved_mlp=True, weight_dtype="mxfp4", mxfp4_weights_only=True)
    assert torch.cuda.memory_allocated() == before  # refused before any weight is built


# ------------------------------------------------------------------------------------------------- engine

PROMPTS_1 = [list(range(10, 10 + n)) for n in (10, 77, 150)]
PROMPTS_2 = [list(range(40, 40 + n)) for n in (300, 21)]


def _engine(weights, **kw):
    from django_assistant_bot_amd.engine.llm_engine import LLMEngine

    args = dict(device=DEV, weights=dict(weights), max_batch=8, block_size=64, num_blocks=64, max_prefill_tokens=256,
                max_model_len=384, use_graphs=True, weight_dtype="mxfp4")
    if "shared_model" in kw:
        del args["weights"], args["weight_dtype"]
    args.update(kw)
    return LLMEngine(TOY, **args)


def _two_waves(eng, first=PROMPTS_1, second=PROMPTS_2, ctx=None):
    """The first prompts, a few decode steps (graph replays), then the second wave: its prefill runs
    between replays of decode graphs that were captured before it."""
    import contextlib

    from django_assistant_bot_amd.engine.llm_engine import SamplingParams

    ctx = ctx or contextlib.nullcontext
    greedy = SamplingParams(max_new_tokens=20, do_sample=False, temperature=0.0, ignore_eos=True)
    with ctx():
        rids = [eng.add_request(p, greedy) for p in first]
        while eng.stats["graph_replays"] < 4:
            eng.step()
        replays = eng.stats["graph_replays"]
        rids += [eng.add_request(p, greedy) for p in second]
        while eng.has_unfinished():
            eng.step()
    assert eng.stats["graph_replays"] > replays + 4
    return [eng.pop_output(r).token_ids for r in rids]


@pytest.mark.parametrize("kv_dtype,stream", [("bf16", True), ("fp8", True), ("bf16", False)])
def test_engine_greedy_tokens_equal_the_two_copy_engine(kv_dtype, stream, monkeypatch):
    """``stream`` off: every GEMM of the captured decode graphs reads the scratch, which the second
    wave's prefill overwrites between their replays."""
    monkeypatch.setattr(LlamaModel, "mxfp4_stream", stream)
    w = _toy_weights(4)
    numels = _numels(w)
    spy = _Spy(monkeypatch)
    outs = {}
    for only in (True, False):
        eng = _engine(w, kv_cache_dtype=kv_dtype, mxfp4_weights_only=only)
        assert eng.mxfp4_weights_only == only == eng.model.mxfp4_weights_only
        st = eng.stats
        assert st["weight_bits"] == 4 and st["weight_bf16_copy"] is (not only)
        assert st["weight_bytes"] == sum(n // 2 + n // 32 + (0 if only else 2 * n) for n in numels)
        assert st["weight_scratch_bytes"] == (2 * max(numels) if only else 0)
        spy.take()
        outs[only] = _two_waves(eng)
        assert (spy.take().get("weight_dequant_mxfp4", 0) > 0) == only
    assert all(len(t) == 20 for t in outs[True]) and outs[True] == outs[False]


def test_two_engines_share_one_model_on_two_streams(monkeypatch):
    monkeypatch.setattr(LlamaModel, "mxfp4_stream", False)  # (the decode graphs read the scratch too)
    w = _toy_weights(4)
    lone = _engine(w, mxfp4_weights_only=True)
    want = _two_waves(lone, PROMPTS_1, PROMPTS_2), _two_waves(lone, PROMPTS_2, PROMPTS_1)
    e1 = _engine(w, mxfp4_weights_only=True)
    e2 = _engine(w, shared_model=e1.model)
    assert e2.mxfp4_weights_only and e2.model is e1.model and e2.stats["weight_scratch_bytes"] == e1.stats["weight_scratch_bytes"]
    from django_assistant_bot_amd.engine.llm_engine import SamplingParams

    greedy = SamplingParams(max_new_tokens=20, do_sample=False, temperature=0.0, ignore_eos=True)
    torch.cuda.synchronize()
    spy = _Spy(monkeypatch)
    streams = torch.cuda.Stream(), torch.cuda.Stream()
    engines = (e1, e2)
    waves = ((PROMPTS_1, PROMPTS_2), (PROMPTS_2, PROMPTS_1))
    rids = [[eng.add_request(p, greedy) for p in waves[i][0]] for i, eng in enumerate(engines)]
    ptrs = [set(), set()]
    second = [False, False]
    while any(eng.has_unfinished() for eng in engines):
        for i, eng in enumerate(engines):
            if not eng.has_unfinished():
                continue
            with torch.cuda.stream(streams[i]):
                eng.step()
            ptrs[i] |= set(spy.outs)
            spy.outs.clear()
            if not second[i] and eng.stats["graph_replays"] >= 4:
                second[i] = True
                rids[i] += [eng.add_request(p, greedy) for p in waves[i][1]]
    torch.cuda.synchronize()
    assert all(second) and all(eng.stats["graph_replays"] > 8 for eng in engines)
    got = tuple([eng.pop_output(r).token_ids for r in rids[i]] for i, eng in enumerate(engines))
    assert got == want
    assert ptrs[0] and ptrs[1] and not (ptrs[0] & ptrs[1])  # each engine dequantised into scratches of its own
