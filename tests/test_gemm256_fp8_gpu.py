"""The FP8-weight arm of gemm256 on the GPU (``ops.gemm256(..., w_exps=)``, ``ops.gemm_bt(..., w_exps=)``, the
candidate epilogue behind ``ops.score_candidates_fp8(..., wide=True)`` and ``VectorIndex(dtype="fp8")``).

Every dequantised weight is a bf16 and a power-of-two scale commutes with fp32 rounding, so the arm must EQUAL the
bf16 ``gemm256`` fragment-layout kernel on ``shuffle_weights(weight_dequantize_fp8(data, exps), group)``: outputs bit
for bit, candidate sets and values entry for entry.  tests/gemm256_fp8_cases.py says why the operands keep that exact.
"""
import numpy as np
import pytest
import torch

import gemm256_fp8_cases as g8
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.vector_index import VectorIndex

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ------------------------------------------------------------------------------------------ C: bit equality


@pytest.mark.parametrize("group", (1, 8))
@pytest.mark.parametrize("M,N,K", g8.G256_SHAPES)
def test_bit_equal_to_the_bf16_kernel(M, N, K, group):
    for epi in g8.EPIS:
        got, want, clean = g8.run_epi(DEV, M, N, K, epi, group)
        assert g8.same_bits(got, want), (M, N, K, group, epi)
        assert clean, (M, N, K, group, epi, "guard rows / columns written")
        assert bool(want.float().abs().sum() > 0)


@pytest.mark.parametrize("epi", g8.EPIS)
def test_bit_equal_where_a_workgroup_walks_two_tiles(epi):
    """272 tiles on 256 CUs with a ragged last row tile: the waits of the first iteration after an epilogue and
    the next tile's prefetch run."""
    M, N, K = g8.G256_BIG
    got, want, clean = g8.run_epi(DEV, M, N, K, epi, 8 if epi == "swiglu8" else 1)
    assert g8.same_bits(got, want) and clean


def test_one_hot_rows_read_the_dequantised_weights():
    """A rows with a single 1.0: the output row is column k of the dequantised weights (one exact product, zeros
    added), the extreme exponent bytes 1 and 254 included.  Pins the byte layout, both k halves of a 64-step and the
    column-to-exponent map without the bf16 kernel."""
    N, K = 512, 384
    data, exps, dq = g8.weights(N, K)
    ks = [0, 9, 18, 27, 33, 36, 45, 54, 63, 64, 127, 128, K // 2 + 7, K - 64, K - 1]
    x = torch.zeros((len(ks), K), dtype=torch.bfloat16)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    want = (dq[:, ks].t() + 0.0).contiguous()  # (+ 0.0: a weight of -0 reads back as the sum 0 + -0 = +0)
    assert {int(exps[r]) for r in g8.EXTREME} == {1, 254} and bool((want[:, list(g8.EXTREME)] != 0).any())
    for group in (1, 8):
        w8, e, _ = g8.copies(N, K, DEV, group)
        y = ops.gemm256(x.to(DEV), w8, shuffled=True, b_group=group, w_exps=e)
        assert g8.same_bits(y.cpu(), want), group


@pytest.mark.parametrize("epi", g8.EPIS)
def test_row_subsets_equal_the_full_calls_rows(epi):
    M, N, K = 513, 512, 384
    full, _, _ = g8.run_epi(DEV, M, N, K, epi, 8)
    g = torch.Generator().manual_seed(3)
    for rows in (torch.randperm(M, generator=g)[:300], torch.tensor([5, 5, 512, 0, 5, 256, 255, 512]),
                 torch.arange(M).flip(0), torch.zeros(0, dtype=torch.long)):
        r = rows.to(torch.int32).to(DEV)
        got, want, clean = g8.run_epi(DEV, M, N, K, epi, 8, rows=r)
        assert clean and g8.same_bits(got, want) and g8.same_bits(got, full[rows.to(DEV)]), (epi, rows.numel())
    # gemm_bt sends rows= / as_m= calls with w_exps to the arm whatever the row count
    w8, e, _ = g8.copies(N, K, DEV, 8)
    A = g8.activations(M, K).to(DEV)
    if epi != "residual":
        code = ops.EPI_SWIGLU8 if epi == "swiglu8" else ops.EPI_NONE
        kw = dict(epilogue=code, shuffled=True, b_group=8, w_exps=e)
        r = torch.tensor([7, 300, 7], dtype=torch.int32, device=DEV)
        assert g8.same_bits(ops.gemm_bt(A, w8, rows=r, **kw), full[r.long()])
        assert g8.same_bits(ops.gemm_bt(A[:40], w8, as_m=M, **kw), full[:40])
        assert g8.same_bits(ops.gemm_bt(A, w8, **kw), full)


def test_two_launches_back_to_back_on_one_stream():
    a = [g8.copies(N, K, DEV, grp) + (g8.activations(M, K).to(DEV),)
         for M, N, K, grp in ((257, 512, 384, 1), (1, 256, 128, 8))]
    want = [ops.gemm256(x, w16, shuffled=True, b_group=grp) for (w8, e, w16, x), grp in zip(a, (1, 8))]
    torch.cuda.synchronize()
    got = [ops.gemm256(x, w8, shuffled=True, b_group=grp, w_exps=e) for (w8, e, w16, x), grp in zip(a, (1, 8))]
    torch.cuda.synchronize()
    assert all(g8.same_bits(g, w) for g, w in zip(got, want))


def test_refusals_launch_nothing(monkeypatch):
    nat = ops.native()
    M, N, K = 64, 256, 128
    w8, e, w16 = g8.copies(N, K, DEV)
    A = g8.activations(M, K).to(DEV)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    launched = []
    real = nat.gemm256_fp8
    monkeypatch.setattr(nat, "gemm256_fp8", lambda *a, **k: launched.append(1) or real(*a, **k))
    bias = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    w8_n, e_n, _ = g8.copies(384, K, DEV)          # N % 256
    w8_k, e_k, _ = g8.copies(N, 192, DEV)          # K % 128
    odd = torch.zeros(N + 1, dtype=torch.uint8, device=DEV)[1:]
    assert odd.data_ptr() % 4
    for kw in (dict(bias=bias), dict(epilogue=ops.EPI_GELU), dict(epilogue=ops.EPI_SWIGLU), dict(shuffled=False),
               dict(B=w8_n, w_exps=e_n), dict(A=A[:, :192].contiguous(), B=w8_k, w_exps=e_k), dict(w_exps=odd),
               dict(w_exps=e[:-4]), dict(B=w16)):
        a = dict(A=A, B=w8, shuffled=True, w_exps=e, out=out)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.gemm256(a.pop("A"), a.pop("B"), **a)
    for kw in (dict(bias=bias), dict(epilogue=ops.EPI_GELU), dict(shuffled=False), dict(n=128), dict(out_f32=True)):
        a = dict(shuffled=True, w_exps=e)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.gemm_bt(A, w8, **a)
    with pytest.raises(ValueError):
        ops.gemm_bt(A, w8_n, shuffled=True, w_exps=e_n)
    assert launched == []
    monkeypatch.undo()
    # the entry point itself: hipErrorInvalidValue before any launch
    s = torch.cuda.current_stream().cuda_stream

    def raw(bias_=0, epi=0, shuf=1, N_=N, K_=K, exps=e.data_ptr()):
        nat.gemm256_fp8(A.data_ptr(), K, w8.data_ptr(), exps, out.data_ptr(), N, bias_, 0, 0, M, N_, K_, epi, s, shuf, 1)

    for kw in (dict(bias_=bias.data_ptr()), dict(epi=1), dict(epi=2), dict(shuf=0), dict(N_=128), dict(K_=64),
               dict(exps=odd.data_ptr()), dict(exps=0)):
        with pytest.raises(RuntimeError, match="gemm256_fp8"):
            raw(**kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    raw()
    assert g8.same_bits(out, ops.gemm256(A, w16, shuffled=True))


# ------------------------------------------------------------------------------------------ candidates


@pytest.mark.parametrize("grouped", (True, False))
@pytest.mark.parametrize("K", g8.CAND_KS)
@pytest.mark.parametrize("M", g8.CAND_MS)
def test_candidates_exact(M, K, grouped):
    """The integer oracle of tests/cand_cases.py on the arm: a ragged half tile (384), n >= N masking inside a tile
    (1000), deleted rows and query groups, a dense query, and lists that overflow (cap = 64)."""
    for N in g8.CAND_NS[:2]:
        got = g8.cand_run(DEV, M, N, K, grouped)
        assert got == [], (M, N, K, grouped, got)


@pytest.fixture(scope="module", params=g8.CAND_KS)
def unit_rows(request):
    """65664 random unit rows of 256 / 768 (257 column tiles: more than one per CU), quantised: (FP8 fragment copy,
    exponents, bf16 fragment copy of the dequantised rows, N, row groups with deleted rows, dequantised rows)."""
    N, K = g8.CAND_NS[2], request.param
    g = torch.Generator(device="cpu").manual_seed(4321)
    v = torch.nn.functional.normalize(torch.randn((N, K), generator=g), dim=-1).to(torch.bfloat16).to(DEV)
    data, exps = ops.kv_quantize(v)
    R = -(-N // 128) * 128
    full = torch.zeros((R, K), dtype=torch.uint8, device=DEV)
    full[:N] = data
    efull = torch.full((R,), 127, dtype=torch.uint8, device=DEV)
    efull[:N] = exps
    deq = ops.weight_dequantize_fp8(full, efull)
    rg = (torch.arange(N, device=DEV) % 5 - 1).to(torch.int32)  # -1: deleted
    return ops.shuffle_weights_fp8(full), efull, ops.shuffle_weights(deq), N, rg, deq


@pytest.mark.parametrize("grouped", (True, False))
@pytest.mark.parametrize("M", g8.CAND_MS)
def test_candidates_equal_the_bf16_candidates_on_the_dequantised_rows(unit_rows, M, grouped):
    """More than 256 tiles, both list forms (M <= 1024: the LDS lists; 1025: per-tile thresholds), thresholds from a
    1/64 row sample (the index's bound for k = 250: lists neither overflow nor stay empty), and one launch whose cap
    the lists overflow: counts, sets and value bits equal ``ops.score_candidates_shuffled``."""
    shuf8, exps, shuf16, N, rg, deq = unit_rows
    K = shuf8.shape[1]
    g = torch.Generator(device="cpu").manual_seed(17 + M)
    q = torch.nn.functional.normalize(torch.randn((M, K), generator=g), dim=-1).to(torch.bfloat16).to(DEV)
    sample = (q.float() @ deq[:N:64].float().t())
    thr = sample.topk(4, dim=1).values[:, -1].contiguous()
    qg = (torch.arange(M, device=DEV) % 5 - 1).to(torch.int32) if grouped else None
    rgs = rg if grouped else None
    for cap in (4096, 32):
        v8, i8, c8 = ops.score_candidates_fp8(q, shuf8, exps, N, thr, cap, rgs, qg, wide=True)
        v16, i16, c16 = ops.score_candidates_shuffled(q, shuf16, N, thr, cap, rgs, qg)
        assert torch.equal(c8, c16)
        if cap == 4096:
            assert 0 < int(c16.max()) <= cap and int((c16 > 0).sum()) > M // 2
            a, b = g8.sorted_lists(v8, i8, c8, cap), g8.sorted_lists(v16, i16, c16, cap)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        else:
            assert int(c16.max()) > cap  # overflow is reported identically


# ------------------------------------------------------------------------------------------ the index


@pytest.mark.parametrize("nq", (128, 300))
def test_index_search_equals_the_grouped_scans(nq, monkeypatch):
    """``VectorIndex(dtype="fp8")`` above one scan launch: ONE launch of the arm, and the result of the scan called
    in groups (the path before the arm)."""
    nat = ops.native()
    dim, rows = 768, 20000
    g = torch.Generator().manual_seed(5)
    idx = VectorIndex(dim, DEV, capacity=rows, dtype="fp8")
    idx.threshold_min_rows = 1024
    idx.add(np.arange(rows, dtype=np.int64), torch.randn((rows, dim), generator=g), doc_ids=np.arange(rows) // 4,
            groups=(np.arange(rows) % 3).astype(np.int32))
    q = torch.randn((nq, dim), generator=g)
    qg = (np.arange(nq) % 4 - 1).astype(np.int32)
    calls = {"arm": 0, "scan": 0}
    real_arm, real_scan = nat.gemm256_candidates_fp8, nat.score_candidates_fp8

    def counted(name, real):
        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f

    monkeypatch.setattr(nat, "gemm256_candidates_fp8", counted("arm", real_arm))
    monkeypatch.setattr(nat, "score_candidates_fp8", counted("scan", real_scan))
    assert nq >= VectorIndex.FP8_WIDE_MIN_M
    before = idx.stats["threshold_searches"]
    got = idx.search(q, 50, q_groups=qg)
    assert calls == {"arm": 1, "scan": 0} and idx.stats["threshold_searches"] == before + 1
    monkeypatch.setattr(VectorIndex, "FP8_WIDE_MIN_M", 1 << 30)  # the scan in groups of 96 queries
    want = idx.search(q, 50, q_groups=qg)
    assert calls == {"arm": 1, "scan": -(-nq // 96)}
    (sa, ia, da), (sb, ib, db) = got, want
    assert sa.shape == sb.shape and torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    distinct = torch.ones_like(sa, dtype=torch.bool)  # (the order among equal scores follows the append order)
    distinct[:, 1:] &= sa[:, 1:] != sa[:, :-1]
    distinct[:, :-1] &= sa[:, 1:] != sa[:, :-1]
    assert torch.equal(ia[distinct], ib[distinct]) and torch.equal(da[distinct], db[distinct])
    assert int(distinct.sum()) > distinct.numel() // 2
