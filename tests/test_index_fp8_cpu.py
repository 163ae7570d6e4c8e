"""The opt-in FP8 vector index without a GPU: the exact operands of tests/index_fp8_cases.py and the checker's
self-test, the FP8 fragment layout's incremental writer, ``VectorIndex`` with FP8 rows on the CPU against a brute-force
oracle over the dequantised rows (search and filters, upsert, remove, compact, growth, snapshots), ``ShardedIndex``
with the dtype, and the dtype parsing (``"fp8"``, ``DAB_INDEX_DTYPE``)."""
import numpy as np
import pytest
import torch

import cand_cases as cc
import index_fp8_cases as fc
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine import vector_index as vi
from django_assistant_bot_amd.engine.vector_index import VectorIndex
from django_assistant_bot_amd.ops import reference as ref
from django_assistant_bot_amd.parallel.sharded_index import ShardedIndex

FP8 = torch.float8_e4m3fn


# ---------------------------------------------------------------------------------------------
# exact operands


@pytest.mark.parametrize("N,K", [(4, 256), (132, 256), (1156, 768)])
def test_scaled_rows_survive_quantisation_exactly(N, K):
    d = fc.data(N, K)
    assert float(d.B.abs().max()) == 8.0
    rows = d.B[:N].to(torch.bfloat16)
    q, e = ref.kv_quantize(rows)
    assert torch.equal(ref.kv_dequantize(q, e), d.B[:N])
    # rows 0, 1, 2 (mod 3) carry 2^0, 2^1, 2^2: three exponent bytes, one apart
    amax = d.B[:N].abs().amax(1)
    for i in range(min(3, N)):
        sel = (torch.arange(N) % 3 == i) & (amax == 2.0 * 2 ** i)
        assert bool(sel.any()) and set(e[sel].tolist()) == {120 + i}
    assert len(set(e.tolist())) >= 3
    # every score is an integer below 2^24, and so is every unscaled sum
    assert torch.equal(d.score.double(), d.A.double() @ d.B[:N].double().t())
    assert int(d.score.abs().max()) < 2 ** 24 and int(fc.unscaled_score(d).abs().max()) < 2 ** 24


@pytest.mark.parametrize("grouped", (True, False))
@pytest.mark.parametrize("M,N,K", [(17, 132, 256), (96, 1156, 768)])
def test_checker_accepts_the_correct_emulation(M, N, K, grouped):
    d = fc.data(N, K)
    assert torch.equal(fc.defective(d, "").score, d.score)
    for dense, cap in ((M > 1, N + 8), (True, 64)):
        thr = cc.thresholds(d, M, dense)
        assert cc.check(fc.emulate(d, M, thr, cap, grouped), d, M, thr, cap, grouped) == []


@pytest.mark.parametrize("defect", ("no_exponent", "swapped_halves", "neighbour_exponent"))
@pytest.mark.parametrize("M,N,K", [(17, 132, 256), (96, 1156, 768)])
def test_checker_rejects_each_planted_defect(M, N, K, defect):
    d = fc.data(N, K)
    thr = cc.thresholds(d, M, dense=True)
    for cap in (N + 8, 64):
        got = cc.check(fc.emulate(d, M, thr, cap, defect=defect), d, M, thr, cap)
        assert got, (defect, cap)


# ---------------------------------------------------------------------------------------------
# layout


def _bytes(n, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ref.kv_quantize(torch.randn((n, k), generator=g).to(torch.bfloat16))


def test_shuffle_rows_into_fp8_matches_the_full_shuffle():
    data, _ = _bytes(96, 192)
    dst = torch.zeros((96, 192), dtype=torch.uint8)
    perm = torch.randperm(96, generator=torch.Generator().manual_seed(1))
    ops.shuffle_rows_into_fp8(dst, perm, data[perm])
    assert torch.equal(dst, ops.shuffle_weights_fp8(data))
    assert torch.equal(ops.unshuffle_weights_fp8(dst), data)


def test_shuffle_rows_into_fp8_leaves_other_rows_alone():
    data, _ = _bytes(64, 128, seed=2)
    base = ops.shuffle_weights_fp8(torch.full((64, 128), 0x5A, dtype=torch.uint8))
    dst = base.clone()
    rows = torch.tensor([0, 5, 17, 31, 32, 63])
    ops.shuffle_rows_into_fp8(dst, rows, data[rows])
    back = ops.unshuffle_weights_fp8(dst)
    assert torch.equal(back[rows], data[rows])
    rest = torch.ones(64, dtype=torch.bool)
    rest[rows] = False
    assert bool((back[rest] == 0x5A).all())
    with pytest.raises(ValueError):
        ops.shuffle_rows_into_fp8(dst.to(torch.int8), rows, data[rows])


def test_index_dequant_blocks_reference():
    data, exps = _bytes(64, 128, seed=3)
    want = ops.shuffle_weights(ops.weight_dequantize_fp8(data, exps))
    out = torch.full((64, 128), -7.0, dtype=torch.bfloat16)
    ops.index_dequant_blocks(ops.shuffle_weights_fp8(data), exps, 1, 3, out, 1)
    assert torch.equal(out[16:48], want[16:48]) and bool((out[:16] == -7).all() and (out[48:] == -7).all())
    with pytest.raises(ValueError):
        ops.index_dequant_blocks(ops.shuffle_weights_fp8(data), exps, 1, 5, out, 1)


# ---------------------------------------------------------------------------------------------
# VectorIndex on the CPU

DIM = 64


def _corpus(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((n, DIM), generator=g)
    ids = np.arange(1000, 1000 + n, dtype=np.int64)
    docs = (np.arange(n) // 3).astype(np.int64)
    groups = (np.arange(n) % 3).astype(np.int32)
    return ids, v, docs, groups


def _brute(idx: VectorIndex, queries, k, q_groups=None, allowed=None, doc_lt=None):
    """Exact top-k over the dequantised live rows, in fp32 from bf16 queries (the CPU path's arithmetic)."""
    n = idx.n
    rows = ref.kv_dequantize(idx.vecs[:n], idx.exps[:n])
    q = torch.as_tensor(queries).float().reshape(-1, idx.dim)
    q = torch.nn.functional.normalize(q, dim=-1).to(torch.bfloat16).float()
    s = q @ rows.t()
    grp, ids, docs = idx.row_group[:n], idx.row_ids[:n], idx.row_docs[:n]
    ok = (grp >= 0)[None, :].expand(len(q), n).clone()
    if q_groups is not None:
        qg = torch.as_tensor(q_groups)[:, None]
        ok &= (qg < 0) | (grp[None, :] == qg)
    if allowed is not None:
        for i, a in enumerate(allowed):
            ok[i] &= torch.isin(ids, torch.as_tensor(sorted(a), dtype=torch.int64))
    if doc_lt is not None:
        ok &= docs[None, :] < torch.as_tensor(doc_lt)[:, None]
    s = torch.where(ok, s, torch.full_like(s, float("-inf")))
    n4 = (max(n, 4) + 3) // 4 * 4  # the score matrix is padded to whole groups of 4 rows (-inf)
    s = torch.cat([s, torch.full((len(q), n4 - n), float("-inf"))], 1)
    ids = torch.cat([ids, torch.full((n4 - n,), -1, dtype=ids.dtype)])
    v, r = torch.topk(s, min(k, n4), dim=1)
    return v, torch.where(torch.isinf(v), torch.full_like(r, -1), ids[r])


def _agree(idx, queries, k, **kw):
    sims, ids, docs = idx.search(queries, k, **kw)
    want_v, want_ids = _brute(idx, queries, k, **kw)
    assert sims.shape == want_v.shape
    assert torch.equal(torch.isinf(sims), torch.isinf(want_v))
    fin = ~torch.isinf(want_v)
    assert torch.allclose(sims[fin], want_v[fin], rtol=0, atol=2e-6)
    # ids wherever the neighbouring similarities are distinct enough for the order to be decided
    gap = torch.ones_like(want_v, dtype=torch.bool)
    gap[:, 1:] &= (want_v[:, :-1] - want_v[:, 1:]).abs() > 1e-5
    gap[:, :-1] &= (want_v[:, :-1] - want_v[:, 1:]).abs() > 1e-5
    assert torch.equal(ids[gap & fin], want_ids[gap & fin])
    assert bool((ids[~fin] == -1).all() and (docs[~fin] == -1).all())
    return sims, ids


def _fp8_index(n=300, capacity=64):
    ids, v, docs, groups = _corpus(n)
    idx = VectorIndex(DIM, "cpu", capacity=capacity, dtype=FP8)
    idx.add(ids, v, doc_ids=docs, groups=groups)
    return idx, ids, v, docs, groups


def test_fp8_rows_are_the_quantised_normalised_rows():
    idx, ids, v, _, _ = _fp8_index()
    assert idx.fp8 and not idx.frag8 and idx.vecs.dtype == torch.uint8 and idx.exps.dtype == torch.uint8
    assert idx.vecs.shape[1] == DIM and idx.exps.shape == (idx.vecs.shape[0],)
    rows = torch.nn.functional.normalize(v, dim=-1).to(torch.bfloat16)
    q, e = ops.kv_quantize(rows)
    assert torch.equal(idx.vecs[:300], q) and torch.equal(idx.exps[:300], e)
    got = idx.rows_data(np.arange(300))
    assert got.dtype == torch.bfloat16 and torch.equal(got.float(), ref.kv_dequantize(q, e))
    assert len(idx) == 300 and idx._cap >= 300  # grew past the capacity of 64


def test_fp8_search_and_filters_on_the_cpu():
    idx, ids, v, docs, groups = _fp8_index()
    q = torch.randn((6, DIM), generator=torch.Generator().manual_seed(5))
    _agree(idx, q, 10)
    _agree(idx, q[0], 10)
    _agree(idx, q, 10, q_groups=[0, 1, 2, -1, 0, 1])
    allowed = [set(ids[i::7].tolist()) for i in range(6)]
    _agree(idx, q, 10, allowed=allowed)
    _agree(idx, q, 10, doc_lt=[5, 50, 100, 1, 0, 99])
    _agree(idx, q, 10, q_groups=[0, 1, 2, -1, 0, 1], allowed=allowed, doc_lt=[50] * 6)
    # a stored row finds itself first
    sims, got, _ = idx.search(v[:4], 1)
    assert got[:, 0].tolist() == ids[:4].tolist() and bool((sims[:, 0] > 0.99).all())


def test_fp8_upsert_remove_compact_and_k_beyond_the_live_rows():
    idx, ids, v, docs, groups = _fp8_index()
    q = torch.randn((4, DIM), generator=torch.Generator().manual_seed(6))
    # upsert: existing ids get new vectors (and two new ids arrive in the same call)
    g = torch.Generator().manual_seed(7)
    new = torch.randn((12, DIM), generator=g)
    up_ids = np.concatenate([ids[:10], [5000, 5001]])
    idx.add(up_ids, new, doc_ids=np.arange(12), groups=np.zeros(12, dtype=np.int32))
    assert len(idx) == 302
    want_q, want_e = ops.kv_quantize(torch.nn.functional.normalize(new, dim=-1).to(torch.bfloat16))
    rows = torch.from_numpy(idx.rows_of(up_ids))
    assert torch.equal(idx.vecs[rows], want_q) and torch.equal(idx.exps[rows], want_e)
    _agree(idx, q, 10)
    # remove, then a forced compact that moves bytes and exponents as they are
    assert idx.remove(ids[20:120]) == 100
    _agree(idx, q, 10)
    live = (idx.row_group[:idx.n] >= 0).nonzero().flatten()
    before = (idx.vecs[live].clone(), idx.exps[live].clone(), idx.row_ids[live].clone())
    idx.compact()
    assert idx.n == 202 == len(idx)
    assert torch.equal(idx.vecs[:202], before[0]) and torch.equal(idx.exps[:202], before[1])
    assert torch.equal(idx.row_ids[:202], before[2])
    _agree(idx, q, 10)
    # k larger than the live rows: every live row, then -inf / -1
    sims, got = _agree(idx, q, 250)
    assert sims.shape == (4, 204) and bool(torch.isinf(sims[:, 202:]).all() and (got[:, 202:] == -1).all())
    assert sorted(got[0, :202].tolist()) == sorted(idx.row_ids[:202].tolist())
    small = VectorIndex(DIM, "cpu", dtype="fp8")
    small.add(ids[:5], v[:5])
    sims, got, _ = small.search(q, 9)
    assert sorted(got[0][~torch.isinf(sims[0])].tolist()) == ids[:5].tolist()


def test_fp8_snapshot_round_trip_is_bit_identical(tmp_path):
    from safetensors import safe_open

    idx, ids, v, docs, groups = _fp8_index()
    idx.remove(ids[3:9])
    path = str(tmp_path / "fp8.safetensors")
    idx.save(path)
    with safe_open(path, framework="pt") as f:
        assert set(f.keys()) == {"vecs_fp8", "exps", "ids", "docs", "group"}
        assert f.metadata()["dtype"] == "float8_e4m3fn" and f.metadata()["dim"] == str(DIM)
        assert f.get_tensor("vecs_fp8").dtype == torch.uint8 and tuple(f.get_tensor("vecs_fp8").shape) == (300, DIM)
        assert torch.equal(f.get_tensor("vecs_fp8"), idx.vecs[:300])
        assert torch.equal(f.get_tensor("exps"), idx.exps[:300])
    back = VectorIndex.load(path, "cpu")
    assert back.dtype == FP8 and back.fp8 and back.n == 300 and len(back) == 294
    assert torch.equal(back.vecs[:300], idx.vecs[:300]) and torch.equal(back.exps[:300], idx.exps[:300])
    q = torch.randn((3, DIM), generator=torch.Generator().manual_seed(8))
    a, b = idx.search(q, 10), back.search(q, 10)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    _agree(back, q, 10)


def test_bf16_snapshot_still_loads_as_bf16(tmp_path, monkeypatch):
    ids, v, docs, groups = _corpus(100)
    idx = VectorIndex(DIM, "cpu")
    assert idx.dtype == torch.bfloat16 and not idx.fp8 and idx.exps is None
    idx.add(ids, v, doc_ids=docs, groups=groups)
    path = str(tmp_path / "bf16.safetensors")
    idx.save(path)
    monkeypatch.setenv("DAB_INDEX_DTYPE", "fp8")  # a snapshot's own dtype wins over the environment
    back = VectorIndex.load(path, "cpu")
    assert back.dtype == torch.bfloat16 and not back.fp8 and torch.equal(back.vecs[:100], idx.vecs[:100])
    q = torch.randn((3, DIM), generator=torch.Generator().manual_seed(9))
    assert all(torch.equal(x, y) for x, y in zip(idx.search(q, 5), back.search(q, 5)))


def test_sharded_index_forwards_the_fp8_dtype(tmp_path):
    ids, v, docs, groups = _corpus(200)
    sh = ShardedIndex(DIM, "cpu", dtype="fp8")
    one = VectorIndex(DIM, "cpu", dtype=FP8)
    sh.add(ids, v, docs, groups)
    one.add(ids, v, docs, groups)
    assert sh.local.fp8 and torch.equal(sh.local.vecs[:200], one.vecs[:200])
    q = torch.randn((5, DIM), generator=torch.Generator().manual_seed(10))
    for kw in ({}, {"q_groups": [0, 1, 2, -1, 0]}):
        assert all(torch.equal(x, y) for x, y in zip(sh.search(q, 10, **kw), one.search(q, 10, **kw)))
    got = sh.search_replicated(q, 10, doc_lt=[40] * 5)
    assert all(torch.equal(x, y) for x, y in zip(got, one.search(q, 10, doc_lt=[40] * 5)))
    assert sh.remove(ids[:7]) == 7
    d = str(tmp_path / "snap")
    sh.save(d)
    back = ShardedIndex.load(d, "cpu")
    assert back.local.fp8 and len(back) == 193
    assert torch.equal(back.local.vecs[:193], sh.local.vecs[:193])
    assert torch.equal(back.local.exps[:193], sh.local.exps[:193])
    assert all(torch.equal(x, y) for x, y in zip(back.search(q, 10), sh.search(q, 10)))


# ---------------------------------------------------------------------------------------------
# dtype parsing


def test_dtype_names():
    assert vi.parse_index_dtype("fp8") == FP8 and vi.parse_index_dtype("float8_e4m3fn") == FP8
    assert vi.parse_index_dtype(FP8) == FP8 and vi.parse_index_dtype(" FP8 ") == FP8
    assert vi.parse_index_dtype("bfloat16") == torch.bfloat16 and vi.parse_index_dtype("bf16") == torch.bfloat16
    assert vi.parse_index_dtype("float32") == torch.float32
    for bad in ("fp4", "nn", ""):
        with pytest.raises(ValueError):
            vi.parse_index_dtype(bad)


def test_environment_variable_only_fills_a_missing_dtype(monkeypatch):
    monkeypatch.delenv("DAB_INDEX_DTYPE", raising=False)
    assert VectorIndex(DIM, "cpu").dtype == torch.bfloat16
    assert ShardedIndex(DIM, "cpu").local.dtype == torch.bfloat16
    monkeypatch.setenv("DAB_INDEX_DTYPE", "fp8")
    assert VectorIndex(DIM, "cpu").dtype == FP8
    assert ShardedIndex(DIM, "cpu").local.dtype == FP8
    assert VectorIndex(DIM, "cpu", dtype=torch.bfloat16).dtype == torch.bfloat16  # the argument wins
    assert VectorIndex(DIM, "cpu", dtype="float32").dtype == torch.float32
    monkeypatch.setenv("DAB_INDEX_DTYPE", "float8_e4m3fn")
    assert VectorIndex(DIM, "cpu").fp8
    monkeypatch.setenv("DAB_INDEX_DTYPE", "fp4")
    with pytest.raises(ValueError):
        VectorIndex(DIM, "cpu")
    monkeypatch.setenv("DAB_INDEX_DTYPE", "")
    assert VectorIndex(DIM, "cpu").dtype == torch.bfloat16


def test_any_width_works_on_the_cpu():
    idx = VectorIndex(24, "cpu", dtype="fp8")
    v = torch.randn((40, 24), generator=torch.Generator().manual_seed(11))
    idx.add(np.arange(40), v)
    sims, ids, _ = idx.search(v[:3], 1)
    assert ids[:, 0].tolist() == [0, 1, 2]
