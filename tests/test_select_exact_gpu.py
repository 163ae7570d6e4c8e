"""The selection kernels of select.hip against the CPU oracle of tests/select_cases.py: every draw is replayed
(the token a row returns is a pure function of seed, counter, row, logits, T, k, p), every greedy tie resolved
to the lowest index, every ``topk_rows`` boundary compared with ``torch.topk``.  tests/test_select_exact_cpu.py
proves the oracle and shows which planted mistake each case rejects.

A row passes if its token is the oracle's; where u lies within DELTA = 2^-14 of a CDF boundary either
neighbour of that boundary passes.  The dyadic rows (64 tied maxima: every term 1.0, u or the top-p cumsum
exactly on a partial sum) are replayed with no DELTA.  Sampled rows advance their counter by exactly 1;
greedy rows (T <= 0) return before the counter is read and leave it as it is, on both kernels.

Kernel instantiation per case, read from the launchers:

    test_draws_replay_the_counter_rng   exact: sample_kernel (select_topk<true>: radix_kth + gather + bitonic sort),
                                        bf16 and fp32 rows.  fast: chunk_topk_kernel<32> (k = kc = 64: the
                                        threshold pre-filter arm) -> sample_merge_kernel, 1 to 16 chunks, a full,
                                        a 1-token (8193) and a 70-token (16454) last chunk.  tp2 / tp8:
                                        sample_candidates on column slices (index_base = slice start; widths 125,
                                        4096 / 4097, 2056 / 2057: the scalar-load arms of bf16 and fp32) ->
                                        sample_merge on the concatenation (ncand 128 .. 1024)
    test_keep_all_rows                  sample_kernel with k = 1024 > V = 1000 (top_k 0) and top_k > V: every
                                        token kept, the radix select at k = n
    test_fast_falls_back_past_16_chunks V = 131,073: ncand = 17 * 64 > 1024, ``sample_tokens(fast=True)`` must
                                        take sample_kernel
    test_dyadic_rows_decide_the_comparisons   all four paths on 64 tied maxima: ``acc > target`` and
                                        ``cum <= thr`` where both sides are equal
    test_chunk_loads_unaligned_and_ragged     chunk_topk_kernel / sample_kernel on rows of 8262 bf16 (odd rows
                                        !vec_ok, even rows a partial last vector), on the view buf[:, 1:1 + V]
                                        of a NaN buffer (every row !vec_ok, bf16 and fp32), on V = 8193 with the
                                        row maximum alone in the second chunk
    test_greedy_ties                    2 / 64 / 1024 tied maxima in one chunk and over all chunks; 1024 in one
                                        chunk overflow the pre-filter's 512 survivors and the chunk's 64 slots:
                                        the radix arm of chunk_topk_kernel, ties taken by ascending index
    test_all_equal_row_is_a_documented_cap    16,454 tied maxima
    test_masked_rows                    mask_logits_kernel (bf16 / fp32, the last, 1-bit mask word), then the draw
    test_topk_rows_boundaries           topk_rows_kernel below n = 32,768, chunk_topk_kernel<32> (fp32; pre-filter
                                        up to k = 64, radix select from 65) -> topk_merge_kernel from there on;
                                        last chunks of 1 and 100 elements (kk < k: (0, -1) padding)

Measured on an MI355X (every case, every path, both launches): no draw differed from the oracle's token, inside
the DELTA band or outside it, so the largest |u - boundary| of a row that differed is 0 (none did); ``__expf``
never moved a draw across a boundary at these shapes.  Share of rows inside the band, the largest over seeds
and counter kinds: 0.59 % for every vocabulary of test_draws_replay_the_counter_rng (the same ladder and the
same draws at every V), 0.78 % keep-all, 0.78 % for the 128-row ragged cases, 1.04 % masked, 0 at V = 131,073;
the dyadic rows sit on their boundaries by construction (half of that launch) and are compared exactly.

Found by these tests and fixed in select.hip with them:

    test_greedy_ties            1024 tied maxima inside one chunk, ``fast=True``: token 8200 for the lowest tied index
                                8195 (bf16 and fp32).  The ties overflow the pre-filter's 512 survivors, and the radix
                                arm of chunk_topk_kernel kept the first 64 tied keys to arrive, not the 64 lowest
                                indices, so the chunk never handed the argmax on.  It now takes tied keys by
                                ascending index whenever more tie than slots are left.
    test_topk_rows_boundaries   n >= 32,768 (two-stage), k 63 .. 1024: "indices among equal values do not ascend" on
                                11 of 18 cases.  topk_merge_kernel ordered equal keys by their place in the candidate
                                list, which the chunk stage's radix arm fills in arrival order; it now orders them
                                by row index, as topk_rows_kernel does.

The all-equal row (16,454 tied maxima, a documented cap: only "the token holds the maximum" is asserted): before
the fix exact returned 0, fast 1536, tp2 1536, tp8 512 and 1024 on its two rows; after it all four paths return 0.

With defects planted one at a time in a scratch build (no address, bound or launch shape changed), the tests
that failed, and the tests of tests/test_kernels_gpu.py and tests/test_sampling_parity_gpu.py on sampling, top-k and
masks (38 of them) that noticed:

    ``row`` left out of sample_kernel's hash            all of test_draws_replay_the_counter_rng, test_keep_all_rows,
                                                        test_fast_falls_back_past_16_chunks, test_dyadic_rows_...,
                                                        test_chunk_loads_..., test_masked_rows (22 cases); earlier tests: none
    sample_merge_kernel reading top_p[0]                the same but the exact-only cases (19 cases); earlier tests: none
    ``acc >= target`` (both kernels)                    test_dyadic_rows_decide_the_comparisons only; earlier tests: none
    bf16 scalar arm of chunk_topk_kernel reading        test_draws_replay_the_counter_rng at V 1000 / 8193 / 16454 bf16 (the
    i0 + e + 1, clamped in range                        tp slices), test_dyadic_rows_...[bf16], test_chunk_loads_... (the three
                                                        bf16 shapes), test_greedy_ties[bf16], test_masked_rows[bf16]; earlier: none
    topk_merge_kernel ordering equal keys by            test_topk_rows_boundaries at n 32768 / 32769 / 32868 with k >= 63
    descending index                                    (15 cases); earlier tests: none
"""
import numpy as np
import pytest
import torch

import select_cases as sc
from django_assistant_bot_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def _params(T, k, p):
    return (torch.from_numpy(T).to(DEV), torch.from_numpy(k).to(DEV), torch.from_numpy(p).to(DEV))


def _replay(logits, oracle, params, paths, seeds=sc.SEEDS, kinds=sc.COUNTERS, tag="", cnt_of=None):
    """Every path x seed x counter kind, two launches each: tokens accepted by the oracle, counters advanced
    by exactly 1 on the sampled rows, the paths agreeing outside the DELTA band."""
    rows = logits.shape[0]
    T, k, p = _params(*params)
    adv = oracle.sampled.astype(np.int64)
    tokens, worst, share = {}, 0.0, 0.0
    for path in paths:
        for seed in seeds:
            for kind in kinds:
                c0 = cnt_of(kind) if cnt_of else sc.counters(kind, rows)
                cnt = torch.from_numpy(c0.copy()).to(DEV)
                for launch in range(2):
                    want_cnt = c0 + launch * adv
                    tok = sc.draw(ops, path, logits, T, k, p, seed, cnt).cpu().numpy()
                    assert np.array_equal(cnt.cpu().numpy(), want_cnt + adv), (path, seed, kind, launch)
                    bad, band, far = sc.check_replay(tok, oracle, seed, want_cnt)
                    assert not bad, (tag, path, seed, kind, launch, bad[:8], tok[bad[:8]],
                                     oracle.expected(seed, want_cnt)[bad[:8]])
                    worst, share = max(worst, far), max(share, band)
                    tokens.setdefault((seed, kind, launch), {})[path] = (tok, want_cnt)
    for (seed, kind, launch), by_path in tokens.items():
        toks = [t for t, _ in by_path.values()]
        cnts = next(iter(by_path.values()))[1]
        inside = np.array([len(a) > 1 for a in oracle.accepted(seed, cnts)])
        for t in toks[1:]:
            assert np.array_equal(t[~inside], toks[0][~inside]), (tag, seed, kind, launch)
    print(f"SELECT-REPLAY {tag} paths={','.join(paths)} band share <= {share:.4f}, "
          f"largest |u - boundary| of a row that differed from the oracle {worst:.3e}")
    return worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", sc.VOCABS)
def test_draws_replay_the_counter_rng(V, dtype):
    logits = sc.make_logits(V).to(DTYPES[dtype]).to(DEV)
    worst = _replay(logits, sc.case_oracle(V), sc.row_params(), sc.PATHS, tag=f"V={V} {dtype}")
    assert worst < sc.DELTA


@pytest.mark.parametrize("dtype", DTYPES)
def test_keep_all_rows(dtype):
    V = 1000
    logits = sc.make_logits(V, steep=True).to(DTYPES[dtype]).to(DEV)
    _replay(logits, sc.keep_all_oracle(V), sc.keep_all_params(V), ("exact",), tag=f"keep-all {dtype}")


def test_fast_falls_back_past_16_chunks():
    V, rows = 131073, 64
    assert ops.kernels.sample_candidates_per_row(V) > 1024
    cpu = sc.make_logits(V, rows=rows)
    oracle = sc.Oracle(cpu, *sc.row_params(rows))
    _replay(cpu.to(torch.bfloat16).to(DEV), oracle, sc.row_params(rows), ("fast", "exact"), seeds=sc.SEEDS[:1],
            tag="V=131073 bf16")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dyadic_rows_decide_the_comparisons(dtype):
    logits = sc.dyadic_logits().to(DTYPES[dtype]).to(DEV)
    _replay(logits, sc.dyadic_oracle(), sc.dyadic_params(), sc.PATHS, seeds=(sc.DYADIC_SEED,), kinds=("dyadic",),
            tag=f"dyadic {dtype}", cnt_of=lambda kind: sc.dyadic_counters())
    # the first launch sits on the boundaries: no DELTA there
    T, k, p = _params(*sc.dyadic_params())
    want = sc.dyadic_oracle().expected(sc.DYADIC_SEED, sc.dyadic_counters())
    for path in sc.PATHS:
        cnt = torch.from_numpy(sc.dyadic_counters()).to(DEV)
        tok = sc.draw(ops, path, logits, T, k, p, sc.DYADIC_SEED, cnt).cpu().numpy()
        assert np.array_equal(tok, want), (path, tok, want)


RAGGED_V = 8192 + 70
RAGGED_ROWS = 128


@pytest.mark.parametrize("shape", ["odd-stride-bf16", "nan-view-bf16", "nan-view-fp32", "one-token-chunk-bf16",
                                   "one-token-chunk-fp32"])
def test_chunk_loads_unaligned_and_ragged(shape):
    rows = RAGGED_ROWS
    dtype = torch.float32 if shape.endswith("fp32") else torch.bfloat16
    if shape.startswith("one-token-chunk"):
        V = 8193
        cpu = sc.make_logits(V, rows=rows, single_top_at_end=True)
        logits = cpu.to(dtype).to(DEV)
        T = sc.row_params(rows)[0]
        top_last = cpu.argmax(1).numpy() == V - 1
        assert top_last[T <= 0].any() and top_last[T > 0].any()  # greedy and sampled
    else:
        V = RAGGED_V
        cpu = sc.make_logits(V, rows=rows)
        if shape == "odd-stride-bf16":
            logits = cpu.to(dtype).to(DEV)
            assert logits.stride(0) * 2 % 16 != 0 and logits.data_ptr() % 16 == 0
        else:
            buf = torch.full((rows + 2, V + 10), float("nan"), dtype=dtype, device=DEV)
            logits = buf[1:rows + 1, 1:1 + V]
            logits.copy_(cpu)
            assert logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 != 0
    oracle = sc.Oracle(cpu, *sc.row_params(rows))
    _replay(logits, oracle, sc.row_params(rows), sc.PATHS, seeds=sc.SEEDS[:1], tag=shape)
    if "view" in shape:
        assert bool(torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all() and torch.isnan(buf[:, 0]).all()
                    and torch.isnan(buf[:, 1 + V:]).all())


TIE_V = 16454


@pytest.mark.parametrize("dtype", DTYPES)
def test_greedy_ties(dtype):
    """torch.argmax semantics: the lowest index among 2, 64 and 1024 tied maxima, in one chunk and over all."""
    cases = [(n, spread) for n in (2, 64, 1024) for spread in (False, True)]
    pos = [sc.tie_positions(TIE_V, n, spread) for n, spread in cases]
    logits = torch.stack([sc.tie_row(TIE_V, q) for q in pos]).to(DTYPES[dtype]).to(DEV)
    rows = len(cases)
    T = torch.zeros(rows, device=DEV)
    k = torch.full((rows,), 50, dtype=torch.int32, device=DEV)
    p = torch.ones(rows, device=DEV)
    want = [int(q[0]) for q in pos]
    got = {}
    for path in sc.PATHS:
        cnt = torch.zeros(rows, dtype=torch.int64, device=DEV)
        got[path] = sc.draw(ops, path, logits, T, k, p, 1, cnt).tolist()
        assert int(cnt.abs().sum()) == 0
    print(f"SELECT-TIES {dtype} want {want} got {got}")
    for path in sc.PATHS:
        assert got[path] == want, (path, cases, got[path], want)


def test_all_equal_row_is_a_documented_cap():
    """More than 1024 tied maxima: ``select_topk`` keeps 1024 of them in arrival order, so the token is a
    maximum but not promised to be index 0."""
    logits = torch.full((2, TIE_V), 3.0, dtype=torch.bfloat16, device=DEV)
    T = torch.zeros(2, device=DEV)
    k = torch.full((2,), 50, dtype=torch.int32, device=DEV)
    p = torch.ones(2, device=DEV)
    for path in sc.PATHS:
        tok = sc.draw(ops, path, logits, T, k, p, 1, torch.zeros(2, dtype=torch.int64, device=DEV)).tolist()
        print(f"SELECT-ALL-EQUAL {path} returned {tok}")
        assert all(0 <= t < TIE_V for t in tok)


@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_rows(dtype):
    cpu, mask, flags, masked, params = sc.masked_case()
    buf = torch.full((sc.MASK_ROWS, sc.MASK_V + 7), 99.0, dtype=DTYPES[dtype], device=DEV)
    logits = buf[:, :sc.MASK_V]
    logits.copy_(cpu)
    out = ops.mask_logits(logits, mask.to(DEV), flags.to(DEV))
    assert out.data_ptr() == logits.data_ptr()
    assert torch.equal(logits.float().cpu(), masked)  # -inf exactly outside the allowed set, bits past V ignored
    assert bool((buf[:, sc.MASK_V:] == 99.0).all())
    _replay(logits, sc.masked_oracle(), params, sc.PATHS, tag=f"masked {dtype}")


def _topk_all_forms(n, k):
    s = sc.topk_scores(n)
    rows = s.shape[0]
    # contiguous, both index widths
    d = s.to(DEV)
    v, i = ops.topk_rows(d, k)
    assert i.dtype == torch.int32
    assert sc.check_topk(v, i, s, k) == []
    v64, i64 = ops.topk_rows(d, k, index_base=sc.TOPK_BASE, want_global=True)
    assert i64.dtype == torch.int64 and torch.equal(v64, v)
    assert sc.check_topk(v64, i64 - sc.TOPK_BASE, s, k) == []
    # (ties at the k-th value are taken in arbitrary order, so two launches may differ there and only there)
    strict = (v > v[:, -1:]).cpu()
    assert torch.equal((i64 - sc.TOPK_BASE)[strict.to(DEV)], i.long()[strict.to(DEV)])
    # a view of a wider buffer whose tail would win every comparison
    big = torch.full((rows + 1, n + 3), float("inf"), device=DEV)
    big[:rows, :n] = d
    v, i = ops.topk_rows(big[:rows, :n], k)
    assert sc.check_topk(v, i, s, k) == []
    # the index's own call: -inf past a per-row count, n_use a multiple of 64 of a wider list
    n_use = n // 64 * 64
    if n_use >= k:
        valid = [k, max(k, n_use - 1), n_use][:rows]
        cpu = s[:, :n_use].clone()
        for r, c in enumerate(valid):
            cpu[r, c:] = float("-inf")
        lists = torch.full((rows, n_use + 64), float("inf"), device=DEV)
        lists[:, :n_use] = cpu.to(DEV)
        v, i = ops.topk_rows(lists[:, :n_use], k)
        assert sc.check_topk(v, i, cpu, k, valid=valid) == []
        assert bool(torch.isfinite(v[0]).all()) and sorted(i[0].tolist()) == list(range(k))  # exactly k valid: all of them


@pytest.mark.parametrize("k", sc.TOPK_KS)
@pytest.mark.parametrize("n", sc.TOPK_NS)
def test_topk_rows_boundaries(n, k):
    assert (n >= 4 * sc.CHUNK) == (n >= 32768)  # the one-stage / two-stage switch
    _topk_all_forms(n, k)
