"""Numerics of every hand-written gfx950 kernel against the plain-PyTorch fp32 reference of the same op."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from django_assistant_bot_amd import ops  # noqa: E402
from django_assistant_bot_amd.ops import reference as ref  # noqa: E402

DEV = "cuda"


def _stream_cases(cfgs, Ms, shapes=((0, 0, 1),)):
    """(cfg, M, N, K, S) combinations a stream_gemm configuration supports (M <= its row limit, N a
    multiple of its tile width), so the parametrised tests below only collect runnable cases.  The
    limits are host-side queries of the built extension; without it every combination is collected
    (and the GPU marker skips them on a CPU host anyway)."""
    try:
        nat = ops.native()
        lim = {c: (nat.stream_gemm_bn(c), nat.stream_gemm_max_m(c)) for c in cfgs}
    except Exception:  # extension not built: no filtering
        lim = {c: (1, 1 << 30) for c in cfgs}
    return [(c, m, n, k, s) for c in cfgs for m in Ms for (n, k, s) in shapes
            if m <= lim[c][1] and (n == 0 or n % lim[c][0] == 0)]


def bf(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16)


def close(a, b, atol=2e-2, rtol=2e-2):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    assert torch.allclose(a, b, atol=atol, rtol=rtol), f"max abs err {err}"


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


def test_native_loaded():
    m = ops.native()
    assert m.__file__.endswith(".so")


@pytest.mark.parametrize("cols", [256, 768, 4096, 8192])
@pytest.mark.parametrize("with_res", [False, True])
def test_rmsnorm(cols, with_res):
    x, w = bf(37, cols), bf(cols)
    r = bf(37, cols) if with_res else None
    out, res = ops.rmsnorm(x, w, 1e-5, residual=r)
    eo, er = ref.rmsnorm(x, w, 1e-5, residual=r)
    close(out, eo)
    if with_res:
        assert torch.equal(res, er)


@pytest.mark.parametrize("cols,rows", [(384, 29), (768, 29), (1024, 29), (768, 4099), (1024, 4096)])
def test_layernorm(cols, rows):
    """Row-per-workgroup kernel (384) and the wave-per-row kernel of the encoder widths (768 / 1024;
    4 rows per workgroup, row counts that do and do not fill the last one)."""
    x, r, g, b = bf(rows, cols), bf(rows, cols), bf(cols), bf(cols)
    close(ops.layernorm(x, g, b, 1e-12, residual=r), ref.layernorm(x, g, b, 1e-12, residual=r))
    close(ops.layernorm(x, g, b, 1e-12), ref.layernorm(x, g, b, 1e-12))


def test_bert_embed_and_pool():
    V, P, H = 500, 64, 768
    word, pos, typ, g, b = bf(V, H), bf(P, H), bf(2, H), bf(H), bf(H)
    ids = torch.randint(0, V, (41,), device=DEV, dtype=torch.int32)
    pids = torch.randint(0, P, (41,), device=DEV, dtype=torch.int32)
    close(ops.bert_embed(ids, pids, None, word, pos, typ, g, b, 1e-12),
          ref.bert_embed(ids, pids, None, word, pos, typ, g, b, 1e-12))
    h = bf(41, H)
    cu = torch.tensor([0, 5, 5, 30, 41], dtype=torch.int32, device=DEV)
    for norm in (False, True):
        got, gotb = ops.mean_pool(h, cu, normalize=norm, want_bf16=True)
        exp = ref.mean_pool(h, cu, norm)
        close(got, exp, atol=1e-3, rtol=1e-3)
        close(gotb, exp)
    close(ops.embed_gather(ids, word), word[ids.long()], atol=0, rtol=0)


def test_gelu_erf_sweep():
    """The epilogue GELU (A&S 7.1.26 erfc, common.h gelu_erf) against torch's exact-erf GELU on every
    bf16 value in [-12, 12]: within one bf16 rounding of the exact result (absolute 2e-7 near 0)."""
    x = torch.arange(-12 * 4096, 12 * 4096, device=DEV, dtype=torch.float32).div(4096).to(torch.bfloat16)
    x = torch.unique(x).reshape(1, -1)
    x = x[:, : x.shape[1] // 8 * 8].contiguous()
    exact = torch.nn.functional.gelu(x.float())
    got = ops.gelu(x).float()
    ulp = exact.abs().clamp_min(1e-30) * 2.0 ** -8
    assert bool(((got - exact).abs() <= ulp + 2e-7).all())


def test_gelu_silu():
    x, b = bf(33, 3072), bf(3072)
    close(ops.gelu(x, b), ref.gelu(x, b))
    y = bf(17, 2 * 1408)
    close(ops.silu_mul(y), ref.silu_mul(y))
    # 16-column interleaved [g16 | u16] layout == the projection of interleave_gate_up weights
    g, u = bf(17, 1408), bf(17, 1408)
    yi = ops.interleave_gate_up(g.t().contiguous(), u.t().contiguous()).t().contiguous()
    close(ops.silu_mul(yi, interleaved=True), ref.silu_mul(torch.cat([g, u], -1)))


@pytest.mark.parametrize("S", [1, 3])
def test_rmsnorm_slabs(S):
    rows, cols = 21, 4096
    slabs = torch.randn(S, rows, cols, device=DEV)
    w, r = bf(cols), bf(rows, cols)
    out, res = ops.rmsnorm(slabs, w, 1e-5, residual=r)
    eo, er = ref.rmsnorm(slabs.sum(0).to(torch.bfloat16), w, 1e-5, residual=r)
    close(out, eo)
    assert torch.equal(res, er)


def test_rope_kv_write():
    T, Hq, Hkv, D, bs, nb = 50, 4, 2, 128, 64, 8
    qkv = bf(T, (Hq + 2 * Hkv) * D)
    inv = ref.llama3_inv_freq(D, 500000.0, {"factor": 8.0})
    cs = ref.rope_cos_sin(inv, 4096).to(DEV)
    pos = torch.randint(0, 4000, (T,), device=DEV, dtype=torch.int32)
    slots = torch.randperm(nb * bs, device=DEV)[:T].to(torch.int64)
    slots[3] = -1
    kc, vc = torch.zeros(nb, Hkv, bs, D, device=DEV, dtype=torch.bfloat16), torch.zeros(nb, Hkv, bs, D, device=DEV,
                                                                                          dtype=torch.bfloat16)
    kr, vr = kc.cpu(), vc.cpu()
    q = ops.rope_kv_write(qkv, pos, cs, kc, vc, slots, Hq, Hkv, D)
    qr = ref.rope_kv_write(qkv.cpu(), pos.cpu(), cs.cpu(), kr, vr, slots.cpu(), Hq, Hkv, D, bs)
    close(q.cpu(), qr)
    close(kc.cpu(), kr)
    assert torch.equal(vc.cpu(), vr)
    # the same through fp32 split-K slabs
    slabs = torch.randn(3, T, (Hq + 2 * Hkv) * D, device=DEV)
    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
    kr2, vr2 = kc2.cpu(), vc2.cpu()
    q2 = ops.rope_kv_write(slabs, pos, cs, kc2, vc2, slots, Hq, Hkv, D)
    qr2 = ref.rope_kv_write(slabs.sum(0).to(torch.bfloat16).cpu(), pos.cpu(), cs.cpu(), kr2, vr2, slots.cpu(), Hq,
                            Hkv, D, bs)
    close(q2.cpu(), qr2)
    close(kc2.cpu(), kr2)
    assert torch.equal(vc2.cpu(), vr2)


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("lens", [[5, 70, 130, 1], [5, 64, 33, 1, 50, 17, 64, 2]])
def test_flash_packed(D, causal, lens):
    """Packed varlen attention against the fp32 reference (long and short, encoder-chunk-like
    batches)."""
    Hq, Hkv = (8, 2) if causal else (4, 4)
    T = sum(lens)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    qkv = bf(T, (Hq + 2 * Hkv) * D)
    q = qkv[:, :Hq * D].view(T, Hq, D)
    k = qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D)
    v = qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)
    out = ops.flash_attention_packed(q, k, v, cu, cu, max(lens), causal=causal)
    exp = ref.flash_attention_packed(q, k, v, cu, cu, causal, 1 / math.sqrt(D))
    close(out, exp)


def _paged_setup(ctx, Hkv, D, bs, nb):
    kc = bf(nb, Hkv, bs, D)
    vc = bf(nb, Hkv, bs, D)
    maxb = max(math.ceil(c / bs) for c in ctx)
    perm = torch.randperm(nb)
    bt = torch.zeros(len(ctx), maxb + 2, dtype=torch.int32)
    o = 0
    for i, c in enumerate(ctx):
        n = math.ceil(c / bs)
        bt[i, :n] = perm[o:o + n].to(torch.int32)
        o += n
    return kc, vc, bt.to(DEV)


@pytest.mark.parametrize("causal", [True, False])
def test_flash_paged_prefill(causal):
    """D = 128 paged prefill (the 32x32-MFMA kernel): ragged query / context lengths, both masks;
    cache slots past each context hold NaN (they must not reach the output)."""
    ctx, qlen = [100, 200, 64, 1000, 33], [30, 64, 64, 257, 33]
    Hq, Hkv, D, bs = 8, 2, 128, 64
    kc, vc, bt = _paged_setup(ctx, Hkv, D, bs, 64)
    btc = bt.cpu()
    for i, c in enumerate(ctx):  # poison the unused tail of each sequence's last block
        if c % bs:
            blk = int(btc[i, c // bs])
            kc[blk, :, c % bs:] = float("nan")
            vc[blk, :, c % bs:] = float("nan")
    q = bf(sum(qlen), Hq, D)
    cu = torch.tensor([0] + list(torch.tensor(qlen).cumsum(0)), dtype=torch.int32, device=DEV)
    ctxt = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    out = ops.flash_attention_paged(q, kc, vc, bt, cu, ctxt, max(qlen), causal=causal)
    kc0, vc0 = kc.nan_to_num(0.0), vc.nan_to_num(0.0)
    exp = ref.flash_attention_paged(q, kc0, vc0, bt, cu, ctxt, causal, 1 / math.sqrt(D))
    assert torch.isfinite(out.float()).all()
    close(out, exp)


@pytest.mark.parametrize("causal", [True, False])
def test_flash_paged_prefill_forced_rescales(causal):
    """The deferred online-softmax rescale (flash_d128, running max kept until a row maximum grows
    by > 2^8) against a full-tensor fp64 reference, with spikes that force both branches: single
    keys aligned with single query rows raise those rows' scores at chosen tiles by +3 (stays under
    the threshold: P up to ~2^4.3 without a rescale) or by +12 / +30 (forces the rescale), in
    different waves and 32-query blocks, the rest of each wave unchanged."""
    ctx = [700, 300]
    qlen = [700, 300]
    Hq, Hkv, D, bs = 8, 2, 128, 64
    kc, vc, bt = _paged_setup(ctx, Hkv, D, bs, 32)
    q = bf(sum(qlen), Hq, D, scale=0.5)
    kc.mul_(0.5)
    btc = bt.cpu()
    # (sequence, query index, key index, score jump in natural-log units)
    spikes = [(0, 650, 70, 3.0), (0, 650, 400, 30.0), (0, 300, 130, 12.0), (0, 40, 10, 30.0), (0, 699, 690, 12.0),
              (1, 250, 200, 3.0), (1, 251, 5, 30.0), (1, 90, 64, 12.0)]
    for si, qi, kj, jump in spikes:
        row = sum(qlen[:si]) + qi
        blk, off = int(btc[si, kj // bs]), kj % bs
        for hk in range(Hkv):
            h = hk * (Hq // Hkv)  # the group's first query head gets the exact jump, the others a side effect
            qv = q[row, h].float()
            kc[blk, hk, off] = (qv * (jump * math.sqrt(D) / qv.pow(2).sum())).to(torch.bfloat16)
    cu = torch.tensor([0] + list(torch.tensor(qlen).cumsum(0)), dtype=torch.int32, device=DEV)
    ctxt = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    out = ops.flash_attention_paged(q, kc, vc, bt, cu, ctxt, max(qlen), causal=causal)
    assert torch.isfinite(out.float()).all()
    o0 = 0
    for b, (n, m) in enumerate(zip(ctx, qlen)):  # fp64 reference over the whole output
        ks = ref.gather_paged(kc, bt[b], n).double().repeat_interleave(Hq // Hkv, dim=1)
        vs = ref.gather_paged(vc, bt[b], n).double().repeat_interleave(Hq // Hkv, dim=1)
        sc = torch.einsum("qhd,khd->hqk", q[o0:o0 + m].double(), ks) / math.sqrt(D)
        if causal:
            qi = torch.arange(m, device=DEV)[:, None] + (n - m)
            sc = sc.masked_fill(torch.arange(n, device=DEV)[None, :] > qi, float("-inf"))
        exp = torch.einsum("hqk,khd->qhd", sc.softmax(-1), vs)
        close(out[o0:o0 + m], exp.float(), atol=2e-2, rtol=2e-2)
        o0 += m


@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (64, 8), (8, 8)])
@pytest.mark.parametrize("split", [False, True])
def test_paged_decode(Hq, Hkv, split):
    ctx = [1, 63, 64, 65, 700, 1500, 2049]
    D, bs = 128, 64
    kc, vc, bt = _paged_setup(ctx, Hkv, D, bs, 128)
    q = bf(len(ctx), Hq, D)
    ctxt = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    ws = ops.DecodeWorkspace(len(ctx), Hq, D, math.ceil(4096 / 512), DEV) if split else None
    out = ops.paged_decode(q, kc, vc, bt, ctxt, 512, ws)
    exp = ref.paged_decode(q, kc, vc, bt, ctxt, 1 / math.sqrt(D))
    close(out, exp)
    if split:  # the in-launch partition combine left its arrival counters at zero for the next call
        assert int(ws.cnt.abs().sum()) == 0
        assert torch.equal(ops.paged_decode(q, kc, vc, bt, ctxt, 512, ws), out)


@pytest.mark.parametrize("M,N,K", [(200, 384, 256), (1, 2304, 768), (513, 1000, 64), (128, 128, 4096)])
def test_gemm_epilogues(M, N, K):
    A, B = bf(M, K), bf(N, K, scale=0.05)
    bias, res = bf(N), bf(M, N)
    close(ops.gemm_bt(A, B), ref.gemm_bt(A, B), atol=3e-2, rtol=2e-2)
    close(ops.gemm_bt(A, B, bias, res), ref.gemm_bt(A, B, bias, res), atol=3e-2, rtol=2e-2)
    close(ops.gemm_bt(A, B, bias, None, ops.EPI_GELU), ref.gemm_bt(A, B, bias, None, ops.EPI_GELU), atol=3e-2,
          rtol=2e-2)
    close(ops.gemm_bt(A, B, out_f32=True), ref.gemm_bt(A, B, out_f32=True), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("M,N,K", [(4100, 3136, 768), (8192, 2304, 256)])
def test_gemm_big_tiles(M, N, K):
    """256x256 / 8-wave path (large M and N), incl. ragged edges."""
    A, B = bf(M, K), bf(N, K, scale=0.05)
    bias, res = bf(N), bf(M, N)
    close(ops.gemm_bt(A, B, bias, res), ref.gemm_bt(A, B, bias, res), atol=3e-2, rtol=2e-2)
    close(ops.gemm_bt(A, B, bias, None, ops.EPI_GELU), ref.gemm_bt(A, B, bias, None, ops.EPI_GELU), atol=3e-2,
          rtol=2e-2)
    x, wg, wu = bf(M, K), bf(N // 2 // 16 * 16, K, scale=0.05), bf(N // 2 // 16 * 16, K, scale=0.05)
    w = ops.interleave_gate_up(wg, wu)
    close(ops.gemm_bt(x, w, epilogue=ops.EPI_SWIGLU), ref.silu_mul(ref.gemm_bt(x, torch.cat([wg, wu], 0))),
          atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 512, 256), (1000, 1024, 512), (4100, 768, 768),
                                   (2048, 2304, 1024), (8192, 2304, 512), (20000, 1024, 128), (9000, 2048, 256),
                                   # production inner dims: Llama-3-8B qkv / o / gate_up (K 4096), down (K 14336),
                                   # bge-base FFN down (K 3072)
                                   (1100, 512, 4096), (600, 256, 14336), (2000, 768, 3072)])
@pytest.mark.parametrize("shuffled", [False, True])
def test_gemm256(M, N, K, shuffled):
    """Phased 256x256 kernel (gemm256.hip) for every eligible shape: ragged M, every epilogue, grids
    of more tiles than CUs (persistent workgroups, next-tile prefetch, counted waits past the
    epilogue stores); B row-major or in the fragment layout the model keeps (one weight copy)."""
    assert ops.native().gemm256_ok(M, N, K, K, K)
    A, B = bf(M, K), bf(N, K, scale=0.05)
    Bk = ops.shuffle_weights(B) if shuffled else B
    g = lambda *a, **k: ops.kernels.gemm256(A, Bk, *a, shuffled=shuffled, **k)  # noqa: E731
    bias, res = bf(N), bf(M, N)
    close(g(), ref.gemm_bt(A, B), atol=3e-2, rtol=2e-2)
    close(g(bias, res), ref.gemm_bt(A, B, bias, res), atol=3e-2, rtol=2e-2)
    close(g(bias, None, ops.EPI_GELU), ref.gemm_bt(A, B, bias, None, ops.EPI_GELU), atol=3e-2, rtol=2e-2)
    close(g(bias), ref.gemm_bt(A, B, bias), atol=3e-2, rtol=2e-2)
    close(g(None, res), ref.gemm_bt(A, B, None, res), atol=3e-2, rtol=2e-2)
    wg, wu = bf(N // 2, K, scale=0.05), bf(N // 2, K, scale=0.05)
    exp = ref.silu_mul(ref.gemm_bt(A, torch.cat([wg, wu], 0)))
    for grp, epi in ((16, ops.EPI_SWIGLU), (8, ops.EPI_SWIGLU8)):
        w = ops.interleave_gate_up(wg, wu, grp)
        got = ops.kernels.gemm256(A, ops.shuffle_weights(w) if shuffled else w, epilogue=epi, shuffled=shuffled)
        close(got, exp, atol=3e-2, rtol=3e-2)
    if not shuffled:
        bg, bu = bf(N // 2), bf(N // 2)
        w = ops.interleave_gate_up(wg, wu)
        bw = ops.interleave_gate_up(bg[:, None], bu[:, None])[:, 0].contiguous()
        close(ops.kernels.gemm256(A, w, bw, epilogue=ops.EPI_SWIGLU),
              ref.silu_mul(ref.gemm_bt(A, torch.cat([wg, wu], 0), torch.cat([bg, bu]))), atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (300, 512, 256), (129, 768, 640), (640, 4096, 4096),
                                   (768, 6144, 4096), (1000, 1024, 14336), (4096, 512, 128), (2048, 2048, 1024),
                                   (384, 28672, 4096), (1, 512, 256), (37, 1024, 512), (128, 4096, 4096),
                                   (187, 28672, 4096)])
def test_gemm_mid(M, N, K):
    """Mid-M stream-K kernel (gemm_mid.hip) against the fp32 reference: ragged M, tiles split over
    1..8 groups (in-launch last-arriver combine), a single iteration, 32 row tiles; plain, residual
    and SwiGLU8 epilogues on the fragment-layout weights.  Bit-reproducible across launches and the
    arrival counters are left at zero."""
    assert ops.kernels.gemm_mid_ok(M, N, K, K)
    A, B = bf(M, K), bf(N, K, scale=0.05)
    Bs = ops.shuffle_weights(B)
    res = bf(M, N)
    exp = ref.gemm_bt(A, B)
    got = ops.kernels.gemm_mid(A, Bs)
    close(got, exp, atol=3e-2, rtol=2e-2)
    close(ops.kernels.gemm_mid(A, Bs, residual=res), ref.gemm_bt(A, B, None, res), atol=3e-2, rtol=2e-2)
    wg, wu = bf(N // 2, K, scale=0.05), bf(N // 2, K, scale=0.05)
    w8 = ops.shuffle_weights(ops.interleave_gate_up(wg, wu, 8))
    close(ops.kernels.gemm_mid(A, w8, epilogue=ops.EPI_SWIGLU8),
          ref.silu_mul(ref.gemm_bt(A, torch.cat([wg, wu], 0))), atol=3e-2, rtol=3e-2)
    for _ in range(3):
        assert torch.equal(ops.kernels.gemm_mid(A, Bs), got)
    torch.cuda.synchronize()
    for slabs, cnt in ops.kernels._MID_WS.values():
        assert int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("variant", [32, 64])
@pytest.mark.parametrize("M,N,K", [(300, 512, 256), (1000, 1024, 4096)])
def test_gemm_mid_k_step_variants(M, N, K, variant):
    """The forced K-steps of gemm_mid: 64 (the 3-stage ring, which is also the default) and 32 (the
    6-stage ring kept as an A/B arm): same numerics contract."""
    A, B = bf(M, K), bf(N, K, scale=0.05)
    Bs = ops.shuffle_weights(B)
    close(ops.kernels.gemm_mid(A, Bs, variant=variant), ref.gemm_bt(A, B), atol=3e-2, rtol=2e-2)
    res = bf(M, N)
    close(ops.kernels.gemm_mid(A, Bs, residual=res, variant=variant), ref.gemm_bt(A, B, None, res), atol=3e-2,
          rtol=2e-2)


def test_gemm_mid_in_a_strided_view_and_out_buffer():
    """A as a row slice of a wider buffer (lda > K) and a caller-provided output view."""
    M, N, K = 700, 1024, 512
    big = bf(M, K + 64)
    A = big[:, :K]
    B = bf(N, K, scale=0.05)
    out_big = torch.zeros((M, N + 256), dtype=torch.bfloat16, device=DEV)
    out = out_big[:, :N]
    ops.kernels.gemm_mid(A, ops.shuffle_weights(B), out=out)
    close(out, ref.gemm_bt(A.contiguous(), B), atol=3e-2, rtol=2e-2)
    assert torch.all(out_big[:, N:] == 0)


@pytest.mark.parametrize("aux", [0, 2, 16, 18])
def test_gemm256_stamped_matches_and_stamps(aux):
    """The diagnostic STAMP instantiation (benchmarks/gemm_stamps.py) computes the same C as the
    production launch, whatever its store cache policy, and leaves one stamp per tile it ran (K-loop
    / epilogue cycles > 0)."""
    from django_assistant_bot_amd.ops.kernels import native, ptr, stream

    M, N, K = 1100, 768, 768  # ragged M, 15 tiles: every workgroup runs 1, some workgroups 0
    A, B, bias, res = bf(M, K), bf(N, K, scale=0.05), bf(N), bf(M, N)
    exp = ops.kernels.gemm256(A, B, bias, res)
    C = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    st = torch.zeros((256, 2, 4), dtype=torch.int32, device=DEV)
    grid = native().gemm256_stamped(ptr(A), K, ptr(B), ptr(C), ptr(bias), ptr(res), M, N, K, 0, 0, ptr(st), 2,
                                    stream(A), aux)
    torch.cuda.synchronize()
    assert torch.equal(C, exp)
    tiles = (M + 255) // 256 * (N // 256)
    s = st[:grid].cpu()
    ran = s[:, :, 0] != 0
    assert int(ran.sum()) == tiles and bool((s[:, :, 2][ran] > 0).all()) and bool((s[:, :, 3][ran] > 0).all())


def test_gemm256_candidates_stamped_matches_production():
    """The stamped candidate-GEMM launcher (benchmarks/gemm_stamps.py --cand) appends the same
    candidate set as the production search path over the same shuffled copy, and stamps every tile."""
    from django_assistant_bot_amd.ops.kernels import native, ptr, stream

    M, N, K = 300, 20_000, 768
    A = torch.nn.functional.normalize(torch.randn(M, K, device=DEV), dim=-1).to(torch.bfloat16)
    B = torch.nn.functional.normalize(torch.randn(N, K, device=DEV), dim=-1).to(torch.bfloat16)
    full = ops.gemm_bt(A, B, epilogue=ops.EPI_SCORES, out_f32=True)
    thr = torch.quantile(full, 0.99, dim=1).contiguous()
    Bp = torch.zeros((-(-N // 128) * 128, K), dtype=torch.bfloat16, device=DEV)
    Bp[:N] = B
    Ws = ops.shuffle_weights(Bp)
    cap = 2048
    cv0, ci0, cnt0 = ops.score_candidates_shuffled(A, Ws, N, thr, cap, None, None)
    cnt = torch.zeros(M, dtype=torch.int32, device=DEV)
    cv = torch.empty(M * cap, dtype=torch.float32, device=DEV)
    ci = torch.empty(M * cap, dtype=torch.int32, device=DEV)
    tiles = (M + 255) // 256 * ((N + 255) // 256)
    per_wg = -(-tiles // 256) + 1
    st = torch.zeros((256, per_wg, 4), dtype=torch.int32, device=DEV)
    grid = native().gemm256_candidates_stamped(ptr(A), K, ptr(Ws), M, N, K, Ws.shape[0], ptr(thr), ptr(cnt), ptr(cv),
                                               ptr(ci), cap, ptr(st), per_wg, stream(A))
    torch.cuda.synchronize()
    assert torch.equal(cnt, cnt0) and int(cnt.max()) <= cap
    ci, cv = ci.view(M, cap), cv.view(M, cap)
    for m in range(0, M, 13):
        k = int(cnt[m])
        assert set(ci[m, :k].tolist()) == set(ci0[m, :k].tolist())
        torch.testing.assert_close(cv[m, :k].sort().values, cv0[m, :k].sort().values, atol=0, rtol=0)
    s = st[:grid].cpu()
    ran = s[:, :, 0] != 0
    assert int(ran.sum()) == tiles and bool((s[:, :, 2][ran] > 0).all())


@pytest.mark.parametrize("shuffled", [False, True])
def test_gemm256_exact_layout(shuffled):
    """Small-integer operands (exact in bf16 and fp32): every output element must match exactly, so a
    swapped row/column map or a misplaced K-slice cannot hide behind the tolerance."""
    M, N, K = 512, 512, 256
    A = torch.randint(-3, 4, (M, K), device=DEV).to(torch.bfloat16)
    B = torch.randint(-2, 3, (N, K), device=DEV).to(torch.bfloat16)
    B[:, 0] += torch.arange(N, device=DEV).to(torch.bfloat16) % 7  # asymmetric in n
    exp = A.float() @ B.float().t()
    got = ops.kernels.gemm256(A, ops.shuffle_weights(B) if shuffled else B, shuffled=shuffled)
    assert torch.equal(got.float(), exp.to(torch.bfloat16).float())


@pytest.mark.parametrize("M,N,K", [(77, 512, 512), (300, 1024, 256), (1000, 2304, 768), (4100, 3136, 768)])
def test_gemm_bt_fragment_layout(M, N, K):
    """The 128x128 / 256x256 kernels of gemm.hip reading B in the fragment layout: plain, residual,
    SwiGLU over 8-row groups, and fp32 filtered scores (the index's generic-filter GEMM)."""
    A, B = bf(M, K), bf(N, K, scale=0.05)
    Bs = ops.shuffle_weights(B)
    res = bf(M, N)
    close(ops.gemm_bt(A, Bs, shuffled=True), ref.gemm_bt(A, B), atol=3e-2, rtol=2e-2)
    close(ops.gemm_bt(A, Bs, residual=res, shuffled=True), ref.gemm_bt(A, B, None, res), atol=3e-2, rtol=2e-2)
    F = N // 32 * 16
    wg, wu = bf(F, K, scale=0.05), bf(F, K, scale=0.05)
    w8 = ops.shuffle_weights(ops.interleave_gate_up(wg, wu, 8))
    close(ops.gemm_bt(A, w8, epilogue=ops.EPI_SWIGLU8, shuffled=True),
          ref.silu_mul(ref.gemm_bt(A, torch.cat([wg, wu], 0))), atol=3e-2, rtol=3e-2)
    rg = torch.randint(-1, 3, (N,), device=DEV, dtype=torch.int32)
    qg = torch.randint(-1, 3, (M,), device=DEV, dtype=torch.int32)
    n = N - 4  # rows past n exist in the copy and must not be scored
    got = ops.gemm_bt(A, Bs, epilogue=ops.EPI_SCORES, out_f32=True, row_group=rg[:n], q_group=qg, shuffled=True, n=n)
    exp = ref.gemm_bt(A, B[:n], epilogue=ops.EPI_SCORES, out_f32=True, row_group=rg[:n], q_group=qg)
    assert got.shape == (M, n) and torch.equal(torch.isinf(got), torch.isinf(exp))
    fin = ~torch.isinf(exp)
    close(got[fin], exp[fin], atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("K,N,act", [(100, 30, None), (70, 257, "gelu"), (768, 766, None)])
def test_linear_pads_odd_widths_onto_the_native_gemm(K, N, act):
    """Widths the MFMA kernels do not tile (K % 64, N % 4) are zero-padded onto them (VERDICT r5
    weak #10: no torch fallback on the GPU); bias, residual and GELU epilogues on the padded call."""
    M = 37
    x, w, b = bf(M, K), bf(N, K, scale=0.05), bf(N)
    res = bf(M, N) if act is None else None
    got = ops.linear(x, w, b, residual=res, act=act)
    assert got.shape == (M, N)
    exp = ref.gemm_bt(x, w, b, res, {None: ops.EPI_NONE, "gelu": ops.EPI_GELU}[act])
    close(got, exp, atol=5e-2, rtol=2e-2)


def test_gemm_swiglu():
    M, F, K = 77, 256, 512
    x, wg, wu = bf(M, K), bf(F, K, scale=0.05), bf(F, K, scale=0.05)
    w = ops.interleave_gate_up(wg, wu)
    got = ops.gemm_bt(x, w, epilogue=ops.EPI_SWIGLU)
    exp = ref.silu_mul(ref.gemm_bt(x, torch.cat([wg, wu], 0)))
    close(got, exp, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("cfg,M,N,K,S", _stream_cases(
    list(range(17)) + [20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37],
    [1, 16, 30, 37, 64, 100, 128, 200, 256],
    [(256, 512, 1), (384, 1024, 4), (128, 1792, 7), (256, 4096, 16), (512, 1280, 1), (672, 512, 1),
     (1344, 1024, 4), (2688, 1792, 7)]))
def test_stream_gemm(cfg, M, N, K, S):
    """Warp-specialised streaming GEMM vs the fp32 reference: bf16 out (+ residual) and fp32 slabs,
    stage counts that do and do not fill the register ring (nst = 1..10)."""
    x, w = bf(M, K), bf(N, K, scale=0.05)
    exp = ref.gemm_bt(x, w, out_f32=True)
    wk = ops.shuffle_weights(w) if ops.native().stream_gemm_shuffled(cfg) else w
    if S == 1:
        close(ops.stream_gemm(x, wk, cfg=cfg), exp.to(torch.bfloat16), atol=3e-2, rtol=2e-2)
        res = bf(M, N)
        close(ops.stream_gemm(x, wk, residual=res, cfg=cfg), ref.gemm_bt(x, w, residual=res), atol=5e-2, rtol=2e-2)
    else:
        slabs = ops.stream_gemm(x, wk, splits=S, cfg=cfg)
        assert slabs.shape == (S, M, N)
        close(slabs.sum(0), exp, atol=1e-2, rtol=1e-2)
        res = bf(M, N)
        close(ops.slab_reduce(slabs, res), ref.gemm_bt(x, w, residual=res), atol=5e-2, rtol=2e-2)


@pytest.mark.parametrize("cfg,M,S", [(10, 128, 8), (10, 100, 4), (13, 64, 8), (30, 5, 4), (27, 200, 8), (20, 128, 2)])
def test_bf16_split_k_slabs_and_their_consumers(cfg, M, S):
    """bf16 split-K slabs (``slab_dtype=bf16``) are the fp32 slabs rounded to bf16, bit for bit; the
    consumers (slab RMSNorm, RoPE / KV write, slab_reduce) sum bf16 slabs exactly as they sum the same
    values held in fp32 (slab order, fp32 adds): bitwise equal outputs."""
    N, K = (1792, 2048) if cfg == 20 else (1024, 2048)
    x, w = bf(M, K), bf(N, K, scale=0.05)
    ws = ops.shuffle_weights(w)
    s32 = ops.stream_gemm(x, ws, splits=S, cfg=cfg, nt=True)
    s16 = ops.stream_gemm(x, ws, splits=S, cfg=cfg, nt=True, slab_dtype=torch.bfloat16)
    assert s16.dtype == torch.bfloat16 and s16.shape == s32.shape
    assert torch.equal(s16, s32.to(torch.bfloat16))
    up = s16.float()  # the bf16 values in fp32 slabs
    g, r = bf(N), bf(M, N)
    a = ops.rmsnorm(s16, g, 1e-5, residual=r)
    b = ops.rmsnorm(up, g, 1e-5, residual=r)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.slab_reduce(s16, r), ops.slab_reduce(up, r))
    # RoPE / KV write over a [S, T, (Hq + 2 Hkv) D] slab stack (8 + 2 x 4 heads of 64)
    Hq, Hkv, D, bs, nb = 8, 4, 64, 64, 4
    qs = s16[:, :, :(Hq + 2 * Hkv) * D].contiguous()
    cs = ref.rope_cos_sin(ref.llama3_inv_freq(D, 500000.0, None), 1024).to(DEV)
    pos = torch.randint(0, 1000, (M,), device=DEV, dtype=torch.int32)
    slots = torch.randperm(nb * bs, device=DEV)[:M].to(torch.int64)
    caches = [torch.zeros(nb, Hkv, bs, D, device=DEV, dtype=torch.bfloat16) for _ in range(4)]
    q16 = ops.rope_kv_write(qs, pos, cs, caches[0], caches[1], slots, Hq, Hkv, D)
    q32 = ops.rope_kv_write(qs.float().contiguous(), pos, cs, caches[2], caches[3], slots, Hq, Hkv, D)
    assert torch.equal(q16, q32) and torch.equal(caches[0], caches[2]) and torch.equal(caches[1], caches[3])


@pytest.mark.parametrize("cfg,M,N,K,S,epi", [(10, 128, 4096, 4096, 8, "none"), (20, 128, 2688, 1024, 1, "swiglu8"),
                                              (20, 100, 28672 // 8, 1024, 1, "swiglu8"), (13, 64, 1792, 2048, 8, "none"),
                                              (30, 5, 1792, 2048, 4, "none"), (30, 16, 2688, 1024, 1, "swiglu8"),
                                              (27, 200, 1792, 2048, 8, "none"), (41, 128, 2688, 1024, 1, "swiglu8"),
                                              (42, 77, 2688, 1024, 1, "swiglu8"), (41, 128, 1792, 2048, 4, "none")])
def test_stream_gemm_grouped_weight_layout(cfg, M, N, K, S, epi):
    """``shuffle_weights(w, G)`` (the G row blocks of a 16 G-row group adjacent per 32-deep k chunk)
    read with ``w_group=G``: the same fragments in a different order, so the output is bit-identical
    to the plain layout's (G = 8, the model's gate_up copy, and G = 7, one per compute wave)."""
    x, w = bf(M, K), bf(N, K, scale=0.05)
    kw = dict(cfg=cfg, nt=True, slab_dtype=torch.bfloat16)
    if epi == "swiglu8":
        kw["epilogue"] = ops.EPI_SWIGLU8
    else:
        kw["splits"] = S
    base = ops.stream_gemm(x, ops.shuffle_weights(w), **kw)
    ran = 0
    for G in (7, 8):
        if N % (16 * G):
            continue
        wg = ops.shuffle_weights(w, G)
        assert torch.equal(ops.unshuffle_weights(wg, G), w)
        assert torch.equal(ops.stream_gemm(x, wg, w_group=G, **kw), base), G
        ran += 1
    assert ran
    if epi == "none":
        close(base.float().sum(0), ref.gemm_bt(x, w, out_f32=True), atol=3e-2, rtol=2e-2)
    if N % 112:
        with pytest.raises(Exception):  # N not a whole number of 7-block groups: refused, not misread
            ops.stream_gemm(x, ops.shuffle_weights(w), w_group=7, **kw)


@pytest.mark.parametrize("M,N,K,path", [(77, 1152, 512, "bt"), (3000, 1152, 768, "bt"), (384, 28672, 4096, "mid"),
                                        (700, 1024, 512, "mid"), (1100, 512, 4096, "256"), (2048, 2304, 1024, "256")])
def test_prefill_gemms_on_the_grouped_weight_layout(M, N, K, path):
    """The prefill GEMMs that read the model's grouped gate_up copy (``shuffle_weights(w, 8)``,
    ``b_group=8``): gemm.hip's 128 / 256 tiles (N % 256 != 0 keeps gemm_mid / gemm256 off), gemm_mid and
    gemm256 -- bit-identical to the same kernel on the plain fragment layout, plain and SwiGLU8."""
    A, B = bf(M, K), bf(N, K, scale=0.05)
    plain, grp = ops.shuffle_weights(B), ops.shuffle_weights(B, 8)
    for epi in (ops.EPI_NONE, ops.EPI_SWIGLU8):
        if path == "bt":
            run = lambda w, g: ops.gemm_bt(A, w, epilogue=epi, shuffled=True, b_group=g)  # noqa: E731
        elif path == "mid":
            run = lambda w, g: ops.kernels.gemm_mid(A, w, epilogue=epi, b_group=g)  # noqa: E731
        else:
            run = lambda w, g: ops.kernels.gemm256(A, w, epilogue=epi, shuffled=True, b_group=g)  # noqa: E731
        got = run(grp, 8)
        assert torch.equal(got, run(plain, 1)), epi
        if epi == ops.EPI_NONE:
            close(got, ref.gemm_bt(A, B), atol=3e-2, rtol=2e-2)
    if path == "bt":
        res = bf(M, N)
        assert torch.equal(ops.gemm_bt(A, grp, residual=res, shuffled=True, b_group=8),
                           ops.gemm_bt(A, plain, residual=res, shuffled=True))


@pytest.mark.parametrize("cfg,S", [(10, 8), (10, 16), (14, 8), (9, 8)])
def test_stream_gemm_slice_per_xcd_mapping(cfg, S):
    """The A/B block mapping that groups K-slices (not tiles) per XCD (``stream_gemm_set_slice_xcd``):
    every (tile, slice) pair is computed exactly once, so the slabs match the default mapping's."""
    M, N, K = 128, 4096, 4096
    x, w = bf(M, K), bf(N, K, scale=0.05)
    ws = ops.shuffle_weights(w)
    base = ops.stream_gemm(x, ws, splits=S, cfg=cfg, nt=True)
    nat = ops.native()
    nat.stream_gemm_set_slice_xcd(1)
    try:
        got = ops.stream_gemm(x, ws, splits=S, cfg=cfg, nt=True)
    finally:
        nat.stream_gemm_set_slice_xcd(0)
    torch.cuda.synchronize()
    assert torch.equal(got, base)
    close(got.sum(0), ref.gemm_bt(x, w, out_f32=True), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("form", ["slabs", "swiglu8", "bf16"])
def test_stream_gemm_consumer_rmsnorm(form, M):
    """Small-batch decode: the consumer GEMM reads the un-normalised residual
    stream and scales row m by rsqrt(mean(x[m]^2) + eps) in its epilogue, the gains folded into W:
    equal to RMSNorm(x) g W^T in fp32 (split-K slabs, the SwiGLU8 gate_up form, plain bf16)."""
    K, eps = 4096, 1e-5
    x = (torch.randn(M, K, device=DEV) * 3).to(torch.bfloat16)
    g = (torch.rand(K, device=DEV) + 0.5).to(torch.bfloat16)
    if form == "swiglu8":
        F = 1024
        wg, wu = bf(F, K, scale=0.02), bf(F, K, scale=0.02)
        w = ops.interleave_gate_up(wg, wu, 8)
    else:
        w = bf(6144 if form == "slabs" else 512, K, scale=0.05)
    wf = (w.float() * g.float()[None]).to(torch.bfloat16)  # gains folded (the model's layout)
    # the kernel's contract: r[m] (x W'^T) with the folded bf16 weights (folding's own rounding is
    # covered by the model-level test against the norm kernels)
    xn = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)
    exp = xn @ wf.float().t()
    ws = ops.shuffle_weights(wf)
    if form == "slabs":
        raw = ops.stream_gemm(x, ws, splits=4, cfg=30, nt=True, norm_eps=eps)
        # per-wave partial sums of squares reduced in wave order: run-to-run bit-reproducible
        assert torch.equal(raw, ops.stream_gemm(x, ws, splits=4, cfg=30, nt=True, norm_eps=eps))
        got = raw.sum(0)
        close(got, exp, atol=5e-2, rtol=2e-2)
    elif form == "swiglu8":
        got = ops.stream_gemm(x, ws, epilogue=ops.EPI_SWIGLU8, cfg=30, nt=True, norm_eps=eps)
        v = exp.view(M, -1, 2, 8)
        close(got, (torch.nn.functional.silu(v[:, :, 0]) * v[:, :, 1]).reshape(M, -1).to(torch.bfloat16),
              atol=5e-2, rtol=3e-2)
    else:
        got = ops.stream_gemm(x, ws, cfg=30, nt=True, norm_eps=eps)
        close(got, exp.to(torch.bfloat16), atol=5e-2, rtol=2e-2)


@pytest.mark.parametrize("cfg,M", [c[:2] for c in _stream_cases([0, 1, 3, 5, 6, 8, 10, 13], [5, 64, 128])])
def test_stream_swiglu_and_strided_x(cfg, M):
    F, K = 512, 1024
    xs, wg, wu = bf(M, K + 64), bf(F, K, scale=0.05), bf(F, K, scale=0.05)
    x = xs[:, :K]  # row stride K + 64
    w = ops.interleave_gate_up(wg, wu)
    if ops.native().stream_gemm_shuffled(cfg):
        w = ops.shuffle_weights(w)
    got = ops.stream_gemm(x, w, epilogue=ops.EPI_SWIGLU, cfg=cfg)
    exp = ref.silu_mul(ref.gemm_bt(x.contiguous(), torch.cat([wg, wu], 0)))
    close(got, exp, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("cfg,M", [c[:2] for c in _stream_cases([10, 13, 20, 21, 22, 23, 30, 31, 41, 42],
                                                                 [5, 30, 64, 128])])
def test_stream_swiglu8(cfg, M):
    """8-row [gate | up] groups (EPI_SWIGLU8, the decode copy of gate_up): BN 96 / 112 / 128 tiles."""
    F, K = 1344, 1024
    x, wg, wu = bf(M, K), bf(F, K, scale=0.05), bf(F, K, scale=0.05)
    w16 = ops.interleave_gate_up(wg, wu)
    w8 = ops.regroup_gate_up(w16, 16, 8)
    assert torch.equal(w8, ops.interleave_gate_up(wg, wu, 8))
    got = ops.stream_gemm(x, ops.shuffle_weights(w8), epilogue=ops.EPI_SWIGLU8, cfg=cfg)
    exp = ref.silu_mul(ref.gemm_bt(x, torch.cat([wg, wu], 0)))
    close(got, exp, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("Q,N", [(5, 3000), (2048, 100004)])
def test_gemm_scores_masks(Q, N):
    K = 768
    q = torch.nn.functional.normalize(torch.randn(Q, K, device=DEV), dim=-1).to(torch.bfloat16)
    x = torch.nn.functional.normalize(torch.randn(N, K, device=DEV), dim=-1).to(torch.bfloat16)
    rg = torch.randint(-1, 3, (N,), device=DEV, dtype=torch.int32)
    qg = torch.tensor([-1, 0, 1, 2, 0] * (Q // 5) + [-1] * (Q % 5), device=DEV, dtype=torch.int32)
    allow = torch.randint(-2 ** 31, 2 ** 31 - 1, (Q, (N + 31) // 32), device=DEV, dtype=torch.int32)
    got = ops.gemm_bt(q, x, epilogue=ops.EPI_SCORES, out_f32=True, row_group=rg, q_group=qg, allow=allow)
    exp = ref.gemm_bt(q, x, epilogue=ops.EPI_SCORES, out_f32=True, row_group=rg, q_group=qg, allow=allow)
    assert torch.equal(torch.isinf(got), torch.isinf(exp))
    fin = ~torch.isinf(exp)
    close(got[fin], exp[fin], atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("n", [5000, 100003])
def test_topk_rows(n):
    s = torch.randn(7, n, device=DEV)
    s[2, 50:] = float("-inf")
    for k in (1, 5, 250, 1024):
        v, i = ops.topk_rows(s, k)
        ev, _ = torch.topk(s, k, dim=-1)
        assert torch.equal(v, ev)
        assert torch.equal(torch.gather(s, 1, i.long()), v)
    v, i = ops.topk_rows(s, 10, index_base=1000, want_global=True)
    assert i.dtype == torch.int64 and int(i.min()) >= 1000


def test_topk_rows_ties_and_prefilter_fallback():
    """Chunk top-k threshold pre-filter (k <= 64): exact values with ties at and above the cut,
    and the radix fallback when too many keys tie with the threshold (all-equal rows)."""
    n = 40000
    s = torch.randn(6, n, device=DEV)
    s[0, ::7] = 2.5                 # ~5.7k equal keys per row, above every other value
    s[1] = 0.0                      # all equal: survivors overflow, radix fallback
    s[2] = torch.randint(0, 3, (n,), device=DEV).float()  # three distinct values
    s[3, 100:] = float("-inf")
    s[4] = torch.round(s[4] * 4) / 4  # coarse grid: many ties at the k-th value
    for k in (1, 7, 50, 64):
        v, i = ops.topk_rows(s, k)
        ev, _ = torch.topk(s, k, dim=-1)
        assert torch.equal(v, ev), k
        assert torch.equal(torch.gather(s, 1, i.long()), v), k
        assert int(i.min()) >= 0 and len(set(i[5].tolist())) == k


@pytest.mark.parametrize("fast", [False, True])
def test_sampling_greedy_and_support(fast):
    V, R = 128256, 64
    logits = torch.randn(R, V, device=DEV).to(torch.bfloat16)
    temp = torch.zeros(R, device=DEV)
    topk = torch.full((R,), 50, dtype=torch.int32, device=DEV)
    topp = torch.full((R,), 0.95, device=DEV)
    cnt = torch.zeros(R, dtype=torch.int64, device=DEV)
    tok = ops.sample_tokens(logits, temp, topk, topp, 123, cnt, fast=fast)
    assert torch.equal(tok.long(), logits.float().argmax(-1))
    temp.fill_(1.0)
    tok = ops.sample_tokens(logits, temp, topk, topp, 123, cnt, fast=fast)
    top50 = torch.topk(logits.float(), 50, dim=-1).indices
    assert bool((top50 == tok.long()[:, None]).any(-1).all())
    assert int(cnt[0]) == 1  # counters advance in-kernel


@pytest.mark.parametrize("fast", [False, True])
def test_sampling_distribution(fast):
    R = 4096
    base = torch.tensor([3.0, 2.0, 1.0, 0.5, -1.0], device=DEV)
    logits = torch.full((R, 1000), -30.0, device=DEV)
    logits[:, :5] = base
    temp = torch.ones(R, device=DEV)
    topk = torch.full((R,), 3, dtype=torch.int32, device=DEV)
    topp = torch.ones(R, device=DEV)
    cnt = torch.arange(R, dtype=torch.int64, device=DEV)
    tok = ops.sample_tokens(logits, temp, topk, topp, 7, cnt, fast=fast).long()
    assert int(tok.max()) <= 2
    freq = torch.bincount(tok, minlength=3).float() / R
    p = torch.softmax(base[:3], 0)
    assert torch.allclose(freq, p, atol=0.03), (freq, p)
    # top-p 0.7 on probs [.665,.245,.09] keeps {0,1}: ascending cumsum .09 <= .3 drops token 2
    topp.fill_(0.7)
    tok = ops.sample_tokens(logits, temp, topk, topp, 7, cnt, fast=fast).long()
    assert int(tok.max()) <= 1


@pytest.mark.parametrize("tp", [2, 4, 8])
@pytest.mark.parametrize("temp_v", [0.0, 1.0])
def test_vocab_parallel_sampling_draws_the_replicated_token(tp, temp_v):
    """with the LM head split by vocabulary over tp ranks, each slice's chunk
    top-64 (``sample_candidates``, ids offset by the slice start) merged by ``sample_merge`` draws
    exactly the token the replicated head's two-stage sampler draws from the full logits, with the
    same counters (top-k 50 -> top-p 0.95 -> multinomial, and greedy)."""
    V, R = 128256, 96
    g = torch.Generator(device=DEV).manual_seed(tp)
    logits = (torch.randn(R, V, device=DEV, generator=g) * 3).to(torch.bfloat16)
    logits[5, 1000:1100] = 9.0  # ties across the top-k boundary, inside one slice
    temp = torch.full((R,), temp_v, device=DEV)
    topk = torch.full((R,), 50, dtype=torch.int32, device=DEV)
    topp = torch.full((R,), 0.95, device=DEV)
    c1 = torch.arange(R, dtype=torch.int64, device=DEV) * 3
    c2 = c1.clone()
    ref = ops.sample_tokens(logits, temp, topk, topp, 99, c1, fast=True)
    Vs = V // tp
    parts = [ops.sample_candidates(logits[:, r * Vs:(r + 1) * Vs].contiguous(), Vs, r * Vs) for r in range(tp)]
    allc = torch.stack(parts, 2).reshape(2, R, -1).contiguous()  # what the all-gather assembles
    got = ops.sample_merge(allc, temp, topk, topp, 99, c2, V)
    assert torch.equal(got, ref)
    assert torch.equal(c1, c2)  # counters advanced once per row either way
    if temp_v == 0.0:
        assert torch.equal(got.long(), logits.float().argmax(-1))


@pytest.mark.parametrize("nq", [1, 7, 20, 37, 300])
@pytest.mark.parametrize("groups", [False, True])
def test_index_threshold_search_matches_full_scan(groups, nq):
    """1 / 7 queries: the persistent LDS-query scan (index_scan.hip); 20: the 128x128 candidate
    kernel; 37: the weight-ring one; 300: the gemm256 G_CAND epilogue (600k rows: partial last tiles)."""
    from django_assistant_bot_amd.engine.vector_index import VectorIndex

    n, dim = 600_000, 256
    g = torch.Generator(device=DEV).manual_seed(5)
    idx = VectorIndex(dim, DEV, capacity=n)
    grp = (torch.arange(n) % 3).numpy().astype("int32") if groups else None
    idx.add(torch.arange(n).numpy(), torch.randn(n, dim, device=DEV, generator=g), groups=grp)
    idx.remove(list(range(0, 5000, 7)))
    q = torch.randn(nq, dim, device=DEV, generator=g)
    qg = [i % 3 if i % 4 else -1 for i in range(nq)] if groups else None
    idx.threshold_search = True
    v1, i1, d1 = idx.search(q, 250, q_groups=qg)
    assert idx.stats["threshold_searches"] == 1 and idx.stats["threshold_overflows"] == 0
    idx.threshold_search = False
    v2, i2, d2 = idx.search(q, 250, q_groups=qg)
    torch.testing.assert_close(v1, v2)
    # same scores; ids may differ only among (fp32-rounding) ties: the candidate lists are in no
    # particular row order and the two paths sum in different kernels.  Where the ids differ the
    # scores agree, and the id sets differ only in rows tied with the k-th score.
    diff = i1 != i2
    torch.testing.assert_close(v1[diff], v2[diff])
    for r in range(nq):
        a, b = set(i1[r].tolist()), set(i2[r].tolist())
        kth = v1[r, -1]
        tied = set(i1[r][(v1[r] - kth).abs() <= 1e-5].tolist()) | set(i2[r][(v2[r] - kth).abs() <= 1e-5].tolist())
        assert (a ^ b) <= tied


@pytest.mark.parametrize("M", [1, 5, 24, 40, 300, 1100])
def test_score_candidates_exact_set(M):
    """Every filtered score >= thr[m] is appended exactly once (the 128x128, streaming and gemm256
    candidate kernels; N not a multiple of 64 / 256)."""
    N, K = 100_004, 256
    A = torch.nn.functional.normalize(torch.randn(M, K, device=DEV), dim=-1).to(torch.bfloat16)
    B = torch.nn.functional.normalize(torch.randn(N, K, device=DEV), dim=-1).to(torch.bfloat16)
    rg = torch.randint(-1, 3, (N,), device=DEV, dtype=torch.int32)
    qg = torch.tensor([(-1 if i % 3 == 0 else i % 3) for i in range(M)], device=DEV, dtype=torch.int32)
    full = ops.gemm_bt(A, B, epilogue=ops.EPI_SCORES, out_f32=True, row_group=rg, q_group=qg)
    thr = torch.quantile(full.clamp_min(-1.0), 0.995, dim=1).contiguous()
    cap = 4096
    cv, ci, cnt = ops.score_candidates(A, B, thr, cap, rg, qg)
    assert int(cnt.max()) <= cap
    for m in range(0, M, max(1, M // 23)):
        k = int(cnt[m])
        got = set(ci[m, :k].tolist())
        exp = set((full[m] >= thr[m]).nonzero().flatten().tolist())
        # scores within an fp32 rounding of the threshold may land on either side
        near = set(((full[m] - thr[m]).abs() < 1e-5).nonzero().flatten().tolist())
        assert (got ^ exp) <= near and len(got) == k
        torch.testing.assert_close(cv[m, :k], full[m, ci[m, :k].long()], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("q", [0.9, 0.999])
def test_score_candidates_gemm256_lds_lists(q):
    """gemm256's candidate epilogue keeps each wave's hits in an LDS list that is flushed at a high-
    water mark and at the kernel end; a tile with more hits than the list holds appends the rest
    directly.  q = 0.9 (~320 hits per wave per tile) drives both; 0.999 the sparse case."""
    M, N, K = 200, 50_000, 256
    A = torch.nn.functional.normalize(torch.randn(M, K, device=DEV), dim=-1).to(torch.bfloat16)
    B = torch.nn.functional.normalize(torch.randn(N, K, device=DEV), dim=-1).to(torch.bfloat16)
    rg = torch.randint(-1, 3, (N,), device=DEV, dtype=torch.int32)
    qg = torch.tensor([(-1 if i % 3 == 0 else i % 3) for i in range(M)], device=DEV, dtype=torch.int32)
    full = ops.gemm_bt(A, B, epilogue=ops.EPI_SCORES, out_f32=True, row_group=rg, q_group=qg)
    thr = torch.quantile(full.clamp_min(-1.0), q, dim=1).contiguous()
    cap = 8192
    cv, ci, cnt = ops.score_candidates(A, B, thr, cap, rg, qg)
    assert int(cnt.max()) <= cap
    for m in range(0, M, 7):
        k = int(cnt[m])
        got = ci[m, :k].tolist()
        exp = set((full[m] >= thr[m]).nonzero().flatten().tolist())
        near = set(((full[m] - thr[m]).abs() < 1e-5).nonzero().flatten().tolist())
        assert len(set(got)) == len(got) == k and (set(got) ^ exp) <= near
        torch.testing.assert_close(cv[m, :k], full[m, ci[m, :k].long()], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("M,K", [(m, 768) for m in (1, 5, 16, 17, 37, 64, 65, 96, 97, 127, 128, 300)] +
                         [(20, 896), (40, 1280), (80, 1280)])
def test_score_candidates_shuffled_exact_set(M, K):
    """The scans over a shuffle_weights copy of the rows (1..96 queries at K 768: index_scan.hip SHUF
    with 1-6 16-query tiles in LDS; 97+: gemm256 G_CAND reading the fragment layout; widths the scan
    does not take: the streaming kernel at <= 64 queries, gemm256 above) append exactly the filtered
    scores >= thr[m] (N not a multiple of 128: the copy is zero-padded)."""
    N = 100_004
    A = torch.nn.functional.normalize(torch.randn(M, K, device=DEV), dim=-1).to(torch.bfloat16)
    B = torch.nn.functional.normalize(torch.randn(N, K, device=DEV), dim=-1).to(torch.bfloat16)
    rg = torch.randint(-1, 3, (N,), device=DEV, dtype=torch.int32)
    qg = torch.tensor([(-1 if i % 3 == 0 else i % 3) for i in range(M)], device=DEV, dtype=torch.int32)
    full = ops.gemm_bt(A, B, epilogue=ops.EPI_SCORES, out_f32=True, row_group=rg, q_group=qg)
    thr = torch.quantile(full.clamp_min(-1.0), 0.995, dim=1).contiguous()
    Bp = torch.zeros((-(-N // 128) * 128, K), dtype=torch.bfloat16, device=DEV)
    Bp[:N] = B
    cap = 4096
    cv, ci, cnt = ops.score_candidates_shuffled(A, ops.shuffle_weights(Bp), N, thr, cap, rg, qg)
    assert int(cnt.max()) <= cap
    for m in range(0, M, max(1, M // 17)):
        k = int(cnt[m])
        got = set(ci[m, :k].tolist())
        exp = set((full[m] >= thr[m]).nonzero().flatten().tolist())
        near = set(((full[m] - thr[m]).abs() < 1e-5).nonzero().flatten().tolist())
        assert (got ^ exp) <= near and len(got) == k
        torch.testing.assert_close(cv[m, :k], full[m, ci[m, :k].long()], atol=1e-5, rtol=1e-5)


def test_index_fragment_layout_tracks_updates():
    """The GPU index keeps its rows ONCE, in the fragment layout; searches of 3 (index_scan), 40
    (streaming GEMM) and 200 queries (8-phase GEMM), the threshold sample and the generic-filter
    score GEMM all read it.  After upserts, fresh rows, removals, a compaction and a capacity growth
    the results equal a row-major index fed the same operations."""
    from django_assistant_bot_amd.engine.vector_index import VectorIndex

    n, dim = 560_000, 256
    g = torch.Generator(device=DEV).manual_seed(9)
    idx = VectorIndex(dim, DEV, capacity=n + 1000)
    plain = VectorIndex(dim, DEV, capacity=n + 1000)
    plain.frag = False
    assert idx.frag

    def add(ids, v):
        idx.add(ids, v)
        plain.add(ids, v)

    add(torch.arange(n).numpy(), torch.randn(n, dim, device=DEV, generator=g))
    q = torch.randn(200, dim, device=DEV, generator=g)

    def check():
        for m in (3, 40, 200):
            v1, i1, _ = idx.search(q[:m], 100)
            v2, i2, _ = plain.search(q[:m], 100)
            torch.testing.assert_close(v1, v2)
            assert (i1 == i2).float().mean() > 0.999
        allowed = [torch.arange(0, n, 7).numpy()] * 5
        v1, i1, _ = idx.search(q[:5], 50, allowed=allowed)
        v2, i2, _ = plain.search(q[:5], 50, allowed=allowed)
        torch.testing.assert_close(v1, v2)
        assert torch.equal(i1, i2)
        rows = torch.arange(0, idx.n, 9973, device=DEV)
        assert torch.equal(idx.rows_data(rows), plain.rows_data(rows))

    check()
    assert idx.stats["threshold_searches"] > 0
    hot = torch.arange(10, 20).numpy()
    add(hot, q[0].repeat(10, 1) + 0.01 * torch.randn(10, dim, device=DEV, generator=g))
    add(torch.arange(n, n + 500).numpy(), torch.randn(500, dim, device=DEV, generator=g))
    check()
    v, i, _ = idx.search(q[:1], 10)
    assert set(i[0].tolist()) == set(hot.tolist())
    for x in (idx, plain):
        x.remove(hot[:5].tolist())
        x.remove(torch.arange(1000, 200_000).numpy())  # > n / 4 dead: compacts
    assert idx.n == plain.n < n
    check()
    add(torch.arange(n + 500, n + 3000).numpy(), torch.randn(2500, dim, device=DEV, generator=g))  # grows
    check()


@pytest.mark.parametrize("lens", [[700, 129, 1], [1000]])
def test_flash_rope_on_load_matches_rope_kernel(lens):
    """Prefill with Q rotated inside the attention (rope_kv_write(write_q=False) + flash(rope=...))
    equals RoPE/KV-write's rotated q fed to the same attention, bit for bit; the caches match too."""
    Hq, Hkv, D, bs = 32, 8, 128, 64
    T = sum(lens)
    g = torch.Generator(device=DEV).manual_seed(3)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=DEV, generator=g).to(torch.bfloat16)
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).to(DEV)
    inv = ref.llama3_inv_freq(D, 500000.0, None)
    cs = ref.rope_cos_sin(inv, 4096).to(DEV)
    nblk = [-(-n // bs) for n in lens]
    bt = torch.zeros((len(lens), max(nblk)), dtype=torch.int32)
    slots, b0 = [], 0
    for i, (n, nb) in enumerate(zip(lens, nblk)):
        bt[i, :nb] = torch.arange(b0, b0 + nb, dtype=torch.int32)
        slots.append(b0 * bs + torch.arange(n))
        b0 += nb
    bt, slots = bt.to(DEV), torch.cat(slots).to(DEV)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    ctx = torch.tensor(lens, dtype=torch.int32, device=DEV)
    caches = [(torch.zeros(b0, Hkv, bs, D, dtype=torch.bfloat16, device=DEV),
               torch.zeros(b0, Hkv, bs, D, dtype=torch.bfloat16, device=DEV)) for _ in range(2)]
    q = ops.rope_kv_write(qkv, pos, cs, caches[0][0], caches[0][1], slots, Hq, Hkv, D)
    a = ops.flash_attention_paged(q, caches[0][0], caches[0][1], bt, cu, ctx, max(lens))
    assert ops.rope_kv_write(qkv, pos, cs, caches[1][0], caches[1][1], slots, Hq, Hkv, D, write_q=False) is None
    b = ops.flash_attention_paged(qkv[:, :Hq * D].view(T, Hq, D), caches[1][0], caches[1][1], bt, cu, ctx, max(lens),
                                  rope=(pos, cs))
    assert torch.equal(caches[0][0], caches[1][0]) and torch.equal(caches[0][1], caches[1][1])
    assert torch.equal(a, b)


@pytest.mark.parametrize("nq", [1, 16, 64, 200])
def test_index_recall_at_250_vs_fp32_oracle(nq):
    """Retrieval quality of the bf16 fragment-layout index at the bench's shape (1M x 768, k=250,
    bge-like unit vectors) against an exact fp32 search of the same corpus: each query has 30
    planted rows at cosine 0.25..0.9 (all must come back, in order) above a random background
    (top-250 boundary ~0.126).  1 query: index_scan; 16: index_scan; 64: streaming GEMM; 200:
    gemm_bt candidates.  The reference searches pgvector in fp32
    (/root/reference/assistant/rag/services/search_service.py:185-196)."""
    from django_assistant_bot_amd.engine.vector_index import VectorIndex

    n, dim, k, plant = 1_000_000, 768, 250, 30
    g = torch.Generator(device=DEV).manual_seed(11)
    X = torch.nn.functional.normalize(torch.randn(n, dim, device=DEV, generator=g), dim=-1)
    q = torch.nn.functional.normalize(torch.randn(nq, dim, device=DEV, generator=g), dim=-1)
    cos = torch.linspace(0.9, 0.25, plant, device=DEV)
    rows = (torch.arange(nq, device=DEV)[:, None] * 4999 + torch.arange(plant, device=DEV) * 31) % n
    r = torch.randn(nq, plant, dim, device=DEV, generator=g)
    r = torch.nn.functional.normalize(r - (r * q[:, None]).sum(-1, keepdim=True) * q[:, None], dim=-1)
    X[rows.flatten()] = (cos[None, :, None] * q[:, None] + (1 - cos * cos).sqrt()[None, :, None] * r).reshape(-1, dim)
    idx = VectorIndex(dim, DEV, capacity=n)
    idx.add(np.arange(n) + 7, X)
    assert idx.frag
    v, ids, _ = idx.search(q, k)
    oracle = torch.mm(q, X.t())  # fp32
    ov, oi = oracle.topk(k, dim=1)
    got = ids - 7
    recall = [len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(got.cpu(), oi.cpu())]
    print(f"recall@250 min {min(recall):.4f} mean {sum(recall) / nq:.4f}")
    assert min(recall) >= 0.97 and sum(recall) / nq >= 0.99
    assert torch.equal(got[:, :plant], rows)  # every planted row, best first
    # returned similarities are the fp32 ones up to bf16 rounding of the operands
    assert (v - oracle.gather(1, got)).abs().max().item() < 3e-3
    assert torch.all(v[:, :-1] >= v[:, 1:])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mask_logits(dtype):
    """JSON-constrained decoding's mask kernel == the CPU masked_fill reference (flagged rows only,
    vocab not a multiple of 32)."""
    rows, V = 37, 128256 + 5
    W = -(-V // 32)
    logits = torch.randn(rows, V, device=DEV).to(dtype)
    mask = torch.randint(-2**31, 2**31 - 1, (rows, W), dtype=torch.int32, device=DEV)
    mask[3] = -1  # all allowed
    flags = (torch.arange(rows, device=DEV) % 3 != 1).to(torch.int32)
    exp = ops.mask_logits(logits.cpu().clone(), mask.cpu(), flags.cpu())
    got = ops.mask_logits(logits.clone(), mask, flags)
    assert torch.equal(got.cpu(), exp)
    assert torch.isinf(got[0]).any() and not torch.isinf(got[1]).any() and not torch.isinf(got[3]).any()


def test_index_threshold_search_overflow_falls_back():
    from django_assistant_bot_amd.engine.vector_index import VectorIndex

    n, dim = 600_000, 64
    idx = VectorIndex(dim, DEV, capacity=n)
    idx.add(torch.arange(n).numpy(), torch.ones(n, dim, device=DEV))  # every score ties: all are candidates
    v, i, _ = idx.search(torch.ones(2, dim, device=DEV), 10)
    assert idx.stats["threshold_overflows"] == 1
    assert torch.allclose(v, torch.ones_like(v), atol=1e-2) and (i >= 0).all()


def test_index_threshold_search_on_clustered_rows_retries_per_chunk():
    """on clustered rows (real embeddings are) far more than k x stride rows clear the
    sample's bound and a candidate list overflows; only the overflowing chunk is retried with the
    capacity it needed (no whole-batch fallback to the [q, n] score matrix), and the result is the
    exact top-k of the full scan."""
    from django_assistant_bot_amd.engine.vector_index import VectorIndex

    g = torch.Generator(device=DEV).manual_seed(3)
    n, dim = 300_000, 128
    center = torch.nn.functional.normalize(torch.randn(dim, device=DEV, generator=g), dim=0)
    # the rows the 1/64 stride sample sees are scattered; every other row sits in the queries'
    # cluster, so nearly all of them clear the sample's k-th best
    vecs = center + 0.05 * torch.randn(n, dim, device=DEV, generator=g)
    vecs[::64] = torch.randn(n // 64 + (n % 64 > 0), dim, device=DEV, generator=g)
    idx = VectorIndex(dim, DEV, capacity=n)
    idx.add(torch.arange(n).numpy(), vecs)
    idx.CAND_BYTES = 8 << 20  # small budget: the 200 queries go through in several chunks
    idx.threshold_min_rows = 1 << 16  # the threshold path at this size (production: from 512k rows)
    qs = center + 0.02 * torch.randn(200, dim, device=DEV, generator=g)
    v, i, _ = idx.search(qs, 250)
    ov = idx.stats["threshold_overflows"]
    assert ov >= 1 and idx.stats.get("threshold_retries", 0) + idx.stats.get("threshold_chunk_full", 0) == ov
    ev, _ = ops.topk_rows(idx.scores(qs), 250)
    assert torch.allclose(v, ev, atol=1e-6), (v - ev).abs().max()


def test_cu_masked_stream_runs_kernels():
    """_native.create_cu_masked_stream: a stream restricted to a CU subset (contiguous low CUs
    excluded) runs native kernels and library GEMMs with the same results (profiles/overlap_probe.md)."""
    nat = ops.native()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    words = (n_cu + 31) // 32
    mask = [0] * words
    for i in range(min(32, n_cu - 1), n_cu):
        mask[i // 32] |= 1 << (i % 32)
    h = nat.create_cu_masked_stream(mask)
    try:
        s = torch.cuda.ExternalStream(h)
        x, w = bf(37, 4096), bf(4096)
        a, b = bf(300, 512), bf(256, 512, scale=0.05)
        exp_n, _ = ops.rmsnorm(x, w, 1e-5)
        exp_g = a.float() @ b.float().t()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            got_n, _ = ops.rmsnorm(x, w, 1e-5)
            got_g = ops.gemm_bt(a, b)
        s.synchronize()
        assert torch.equal(got_n, exp_n)
        close(got_g, exp_g, atol=3e-2, rtol=2e-2)
    finally:
        torch.cuda.synchronize()
        nat.destroy_stream(h)


@pytest.mark.parametrize("ctx,qlen", [([4096, 6000], [512, 1024]), ([8192], [8192]), ([8192, 5000], [1, 700]),
                                      ([9000], [300])])
def test_flash_paged_prefill_long_context_llama_heads(ctx, qlen):
    """Llama-3-8B head layout (Hq 32, Hkv 8, D 128) at 4K-8K context: chunked prefill (q = the last
    qlen positions of ctx) and a full 8K prompt, against the fp32 reference."""
    Hq, Hkv, D, bs = 32, 8, 128, 64
    nb = sum(math.ceil(c / bs) for c in ctx) + 4
    kc, vc, bt = _paged_setup(ctx, Hkv, D, bs, nb)
    q = bf(sum(qlen), Hq, D)
    cu = torch.tensor([0] + list(torch.tensor(qlen).cumsum(0)), dtype=torch.int32, device=DEV)
    ctxt = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    out = ops.flash_attention_paged(q, kc, vc, bt, cu, ctxt, max(qlen), causal=True)
    exp = ref.flash_attention_paged(q, kc, vc, bt, cu, ctxt, True, 1 / math.sqrt(D))
    close(out, exp)


@pytest.mark.parametrize("part", [512, 2048])
@pytest.mark.parametrize("split", [False, True])
def test_paged_decode_8k_context(part, split):
    """Decode at the engine's full 8192-token context (max_position of Llama-3), with the split-K
    partition sizes the engine uses (512 for small batches, 2048 at RAG batch sizes)."""
    ctx = [8192, 8191, 5000, 4097, 2048, 1]
    Hq, Hkv, D, bs = 32, 8, 128, 64
    nb = sum(math.ceil(c / bs) for c in ctx) + 4
    kc, vc, bt = _paged_setup(ctx, Hkv, D, bs, nb)
    q = bf(len(ctx), Hq, D)
    ctxt = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    ws = ops.DecodeWorkspace(len(ctx), Hq, D, math.ceil(8192 / part), DEV) if split else None
    out = ops.paged_decode(q, kc, vc, bt, ctxt, part, ws)
    exp = ref.paged_decode(q, kc, vc, bt, ctxt, 1 / math.sqrt(D))
    close(out, exp)
    # longest-first dispatch order: same result (each item writes its own sequence's rows)
    order = torch.argsort(ctxt, descending=True).to(torch.int32)
    assert torch.equal(ops.paged_decode(q, kc, vc, bt, ctxt, part, ws, order=order), out)
    # any other permutation too: the partition bound is the kernel's own max over ctx_lens, so an
    # order that does not start at the longest context skips nothing
    for order in (torch.argsort(ctxt).to(torch.int32), torch.tensor([5, 2, 0, 4, 1, 3], dtype=torch.int32, device=DEV)):
        assert torch.equal(ops.paged_decode(q, kc, vc, bt, ctxt, part, ws, order=order), out)


def test_empty_batches_on_gpu():
    """Zero-row inputs (a rank whose sharded-search batch is empty) return empty results instead of
    tripping the contiguity checks: an empty view's strides are arbitrary."""
    from django_assistant_bot_amd.engine.vector_index import VectorIndex

    cand = torch.zeros((0, 80, 3), dtype=torch.int32, device="cuda")
    cs = cand[..., 0].view(torch.float32).contiguous()
    v, i = ops.topk_rows(cs, 40)
    assert v.shape == (0, 40) and i.shape == (0, 40)
    idx = VectorIndex(256, "cuda")
    idx.add(np.arange(300), torch.randn(300, 256))
    s, ids, docs = idx.search(torch.zeros((0, 256)), 10)
    assert s.shape == (0, 10) and ids.shape == (0, 10)


@pytest.mark.parametrize("B,blocks", [(1, 192), (4, 64), (16, 1)])
def test_paged_decode_l3_warm_leaves_the_output_unchanged(B, blocks):
    """Workgroups appended to the small-batch decode attention warm two weight ranges into the
    Infinity Cache (``warm=``); the attention's output and its arrival counters are bit-identical."""
    ctx = [1100 + 37 * i for i in range(B)]
    Hq, Hkv, D, bs = 32, 8, 128, 64
    nb = sum(math.ceil(c / bs) for c in ctx) + 4
    kc, vc, bt = _paged_setup(ctx, Hkv, D, bs, nb)
    q = bf(B, Hq, D)
    ctxt = torch.tensor(ctx, dtype=torch.int32, device=DEV)
    ws = ops.DecodeWorkspace(B, Hq, D, math.ceil(4096 / 512), DEV)
    base = ops.paged_decode(q, kc, vc, bt, ctxt, 512, ws)
    w0, w1 = bf(4096, 4096), bf(1000, 4096)  # o-sized, then a partial range of a second tensor
    for ranges in ([(w0, w0.numel() * 2)], [(w0, w0.numel() * 2), (w1, 3 << 20)], [(w1, 4096 * 16)]):
        out = ops.paged_decode(q, kc, vc, bt, ctxt, 512, ws, warm=(ranges, blocks))
        torch.cuda.synchronize()
        assert torch.equal(out, base)
        assert int(ws.cnt.abs().sum()) == 0
    with pytest.raises(Exception):
        ops.paged_decode(q, kc, vc, bt, ctxt, 512, ws, warm=([(w1, 100)], blocks))  # not a 16-B multiple


@pytest.mark.parametrize("env,val", [("DAB_ENC_W5", "1"), ("DAB_FLASH_W8", "1"), ("DAB_FLASH_W8", "2"),
                                     ("DAB_FLASH_PAIR", "0"), ("DAB_FLASH_G", "3"), ("DAB_FLASH_1BAR", "1"),
                                     ("DAB_FLASH_Q64", "1"), ("DAB_ENC_PERSIST", "1"), ("DAB_FLASH_SMS", "1"),
                                     ("DAB_FLASH_SGB", "1"), ("DAB_FLASH_LPT", "0"), ("DAB_FLASH_G", "5")])
def test_attention_variants_match_the_default_kernel(env, val, monkeypatch):
    """Occupancy / pipeline variants of the attention kernels selected per launch by environment
    switch (the A/B arms of benchmarks/kernel_bench.py attn) produce the default kernel's output:
    the 5-waves-per-SIMD encoder kernel bit for bit, the 8-wave 3-deep-ring prefill kernel
    (a different wave -> query mapping, same per-query math) bit for bit as well, and so does the
    paired-block causal kernel (both blocks of a pair, odd block counts, a 1-token sequence)."""
    g = torch.Generator().manual_seed(3)
    if env in ("DAB_ENC_W5", "DAB_ENC_PERSIST"):
        lens = torch.randint(20, 140, (37,), generator=g)
        cu = torch.zeros(38, dtype=torch.int32)
        cu[1:] = torch.cumsum(lens, 0)
        T, H, D = int(cu[-1]), 12, 64
        qkv = bf(T, 3 * H * D)
        q, k, v = (qkv[:, i * H * D:(i + 1) * H * D].view(T, H, D) for i in range(3))
        cu = cu.to(DEV)
        run = lambda: ops.flash_attention_packed(q, k, v, cu, cu, int(lens.max()))  # noqa: E731
        exp = ref.flash_attention_packed(q, k, v, cu, cu, False, 1 / math.sqrt(D))
    else:
        ctx = [1, 100, 255, 256, 257, 700, 1024, 1500]
        Hq, Hkv, D, bs = 32, 8, 128, 64
        nb = sum(math.ceil(c / bs) for c in ctx) + 4
        kc, vc, bt = _paged_setup(ctx, Hkv, D, bs, nb)
        cu = torch.zeros(len(ctx) + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(torch.tensor(ctx), 0)
        q = bf(int(cu[-1]), Hq, D)
        cu, ctxt = cu.to(DEV), torch.tensor(ctx, dtype=torch.int32, device=DEV)
        run = lambda: ops.flash_attention_paged(q, kc, vc, bt, cu, ctxt, max(ctx), causal=True)  # noqa: E731
        exp = None
    # (PAIR and the heaviest-first walk are the default: their arms turn them off; DAB_FLASH_G=3 / 5
    # walk 3 / 5 pairs per workgroup against 1)
    monkeypatch.setenv(env, {"0": "1", "3": "1", "5": "1"}.get(val, "0"))
    base = run()
    monkeypatch.setenv(env, val)
    out = run()
    torch.cuda.synchronize()
    if env == "DAB_FLASH_SMS":  # (the row sum in slice order: equal to within a bf16 rounding)
        close(out, base, atol=1e-2, rtol=1e-2)
    else:
        assert torch.equal(out, base)
    if exp is not None:
        close(out, exp)
