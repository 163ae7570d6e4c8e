"""The oracle of tests/select_cases.py, proved on the CPU: its keys and counter RNG against known values, its
kept sets and probabilities against HF's own logits warpers and ``ops.reference.sample_hf``, the conditions
under which an fp32 kernel and the fp64 oracle must draw the same token, and -- mistake by mistake -- which
case of tests/test_select_exact_gpu.py rejects each planted defect.

Conditions (asserted, not measured), for every vocabulary of the replay cases:

    rows inside the DELTA band        <= 2 % of a launch (<= 64 kept tokens: the band covers <= 64 * 2 DELTA = 0.8 %;
                                      the rows that keep all 1000 tokens have a steep tail, under 1e-6 of the mass: 0.8 % at most)
    top-p prefix sums                 none within 1e-4 relative of (1 - p) * total, so ``keep`` is the same in
                                      fp32 and fp64 (the dyadic rows sit exactly on it, in exact arithmetic)
    kept logits                       every value is exact in bf16, so none that should differ share one

Planted mistakes on the oracle side and the case that separates each (rows whose token leaves the accepted set):

    row out of the hash               every replay case: with all counters 0, every row would draw one u
    counter + 1 used for the draw     every replay case
    >= for > in the pick              the dyadic rows (u exactly on a partial sum); no random row can decide it
    cum < thr for <= in top-p         the dyadic rows with top_p 0.5 (32 of 64 equal tokens: the cumsum is thr)
    ties not extended                 the rows whose ranks 2 and 3 tie under top_k 3 (and ranks 47..52 under 50)
    ties extended over -inf           changes no draw: a -inf logit has probability 0 in every precision, which
                                      this module asserts; the kernel's guard saves the walk over 1024 dead
                                      candidates, so this one is not observable in a token
    the neighbouring row's top_k      every replay case (neighbouring rows never share top_k)
    highest instead of lowest tie     the greedy tie rows
"""
import numpy as np
import pytest
import torch

import select_cases as sc
from django_assistant_bot_amd.ops import reference as ref


def test_keys_order_and_round_trip():
    f = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 0.125, 12.0, np.inf], dtype=np.float32)
    k = sc.float_key(f)
    assert k[0] == 0x007FFFFF and k[4] == 0x80000000 and k[3] == 0x7FFFFFFF  # kNegInfKey; +0.0; -0.0 just below
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert np.array_equal(sc.key_float(k).view(np.uint32), f.view(np.uint32))
    rnd = np.random.default_rng(0).standard_normal(10000).astype(np.float32)
    order = np.argsort(rnd, kind="stable")
    assert np.all(np.diff(sc.float_key(rnd)[order].astype(np.int64)) >= 0)
    assert np.array_equal(sc.key_float(sc.float_key(rnd)), rnd)


def test_counter_rng():
    assert sc.splitmix64(0) == 0xE220A8397B1DCDAF  # the published first output of SplitMix64 seeded with 0
    assert sc.splitmix64((1 << 64) - 1) == sc.splitmix64(-1 & ((1 << 64) - 1))
    # the product counter * constant wraps: 2^64 / gcd is no period of interest, but the wrap must be mod 2^64
    big = (1 << 62) + 1
    assert sc.draw_u(3, big, 9) == sc.draw_u(3, big + (1 << 64), 9)
    us = np.array([sc.draw_u(s, c, r) for s in sc.SEEDS for c in (0, 1, big) for r in range(64)])
    assert us.min() >= 0 and us.max() < 1 and np.array_equal(us * 2 ** 24, np.floor(us * 2 ** 24))
    assert np.unique(us).size == us.size  # seed, counter and row all reach the hash
    # the vectorised form used to search boundary draws is the same function
    cnt = np.array([0, 1, 77, (1 << 32) + 5, big], dtype=np.int64)
    assert np.array_equal(sc.draws_np(11, cnt, 5), np.array([sc.draw_u(11, int(c), 5) for c in cnt]))
    assert 0.49 < np.mean(sc.draws_np(11, np.arange(100000), 0)) < 0.51


def _hf_probs(row, temp, k, p):
    from transformers.generation.logits_process import (TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)

    x = row[None].clone()
    if temp != 1.0:
        x = TemperatureLogitsWarper(float(temp))(None, x)
    if 0 < k:
        x = TopKLogitsWarper(top_k=int(k))(None, x)
    if p < 1.0:
        x = TopPLogitsWarper(top_p=float(p))(None, x)
    return torch.softmax(x.double(), -1)[0]


def _oracle_probs(o: sc.RowOracle, V: int) -> torch.Tensor:
    out = torch.zeros(V, dtype=torch.float64)
    out[torch.from_numpy(o.idx)] = torch.from_numpy(np.diff(o.cdf, prepend=0.0))
    return out


@pytest.mark.parametrize("V", [1000, 8193])
def test_oracle_matches_hf_warpers(V):
    pytest.importorskip("transformers")
    logits, (T, k, p) = sc.make_logits(V), sc.row_params()
    orc = sc.case_oracle(V)
    seen = set()
    for r in range(sc.R):
        if T[r] <= 0:
            continue
        want = _hf_probs(logits[r], T[r], k[r], p[r])
        got = _oracle_probs(orc.rows[r], V)
        assert set(torch.nonzero(want).flatten().tolist()) == set(orc.rows[r].idx.tolist()), r
        assert float((want - got).abs().max()) < 1e-6, r
        seen.add((float(T[r]), int(k[r]), float(p[r]), r % 5))
    assert len(seen) == 3 * 4 * 3 * 5  # the sampled (T, k, p) grid times the ladder kinds
    # rows that keep everything: top_k 0 (HF: no top-k warper) and top_k > V (HF clamps it to V)
    if V == 1000:
        logits, (T, k, p) = sc.make_logits(V, steep=True), sc.keep_all_params(V)
        orc = sc.keep_all_oracle(V)
        for r in range(0, 60):
            want = _hf_probs(logits[r], T[r], min(int(k[r]), V), p[r])
            assert float((want - _oracle_probs(orc.rows[r], V)).abs().max()) < 1e-6, r


def test_oracle_matches_reference_sampler():
    """``ops.reference.sample_hf`` draws with torch.multinomial, so it is compared as a distribution:
    4,000 draws of three rows against the oracle's probabilities, and exactly on the greedy rows."""
    V = 1000
    logits, (T, k, p) = sc.make_logits(V), sc.row_params()
    orc = sc.case_oracle(V)
    g = torch.Generator().manual_seed(3)
    for r in (1, 6, 11):  # T 0.7 / top_k 3 / p 1.0 (tied), T 1.0 / 50 / 0.5, T 1.3 / 3 / 1.0
        n = 4000
        tok = ref.sample_hf(logits[r][None].expand(n, -1), torch.full((n,), float(T[r])), torch.full((n,), int(k[r])),
                            torch.full((n,), float(p[r])), g).long()
        freq = torch.bincount(tok, minlength=V).double() / n
        want = _oracle_probs(orc.rows[r], V)
        assert set(torch.nonzero(freq).flatten().tolist()) <= set(orc.rows[r].idx.tolist())
        assert 0.5 * float((freq - want).abs().sum()) <= 0.03, r
    greedy = np.nonzero(T <= 0)[0][:40]
    got = ref.sample_hf(logits[greedy], torch.from_numpy(T[greedy]), torch.from_numpy(k[greedy]),
                        torch.from_numpy(p[greedy]))
    assert got.tolist() == [int(orc.rows[r].idx[0]) for r in greedy]


def test_top_p_keeps_at_least_one_and_top_k_is_capped():
    x = np.full(2000, -4.0, dtype=np.float32)
    x[5], x[700] = 9.0, 1.0
    o = sc.row_oracle(x, 1.0, 50, 1e-6)
    assert o.idx.tolist() == [5] and o.cdf.tolist() == [1.0]
    o = sc.row_oracle(x, 1.0, 0, 1.0)       # 1998 ties at the 1024th value: the cap holds
    assert o.idx.size == sc.CAP and o.idx[:2].tolist() == [5, 700] and np.all(np.diff(o.idx[2:]) > 0)
    x[100:] = -np.inf                        # a masked row: 2 + 98 finite
    x[5] = 9.0
    o = sc.row_oracle(x, 1.0, 200, 1.0)
    assert o.idx.size == 100 and o.idx[0] == 5


@pytest.mark.parametrize("V", sc.VOCABS)
def test_replay_conditions(V):
    logits = sc.make_logits(V)
    assert torch.equal(logits.to(torch.bfloat16).float(), logits)
    T, k, p = sc.row_params()
    assert len({(a, b, c) for a, b, c in zip(T.tolist(), k.tolist(), p.tolist())}) == 48
    assert np.all(k[1:] != k[:-1])
    orc = sc.case_oracle(V)
    margins = np.array([o.top_p_margin for o in orc.rows])
    print(f"SELECT-COND V={V} smallest top-p margin {margins.min():.3e}, most kept {max(o.idx.size for o in orc.rows)}")
    assert margins.min() > 1e-4
    assert max(o.idx.size for o in orc.rows) <= 64  # 60 ladder + 4 background under top_k 64
    kept = {(int(k[r]), r % 5): orc.rows[r].idx.size for r in range(sc.R) if T[r] > 0 and p[r] == 1.0}
    assert kept[(50, 1)] == 53 and kept[(3, 2)] == 4 and kept[(50, 0)] == 50 and kept[(64, 0)] == 64
    for seed in sc.SEEDS:
        for kind in sc.COUNTERS:
            cnt = sc.counters(kind)
            share = orc.band_share(seed, cnt)
            print(f"SELECT-COND V={V} seed={seed:#x} counters={kind} band share {share:.4f}")
            assert share <= 0.02
            assert orc.band_share(seed, cnt + 1) <= 0.02  # the second launch


def test_keep_all_conditions():
    orc = sc.keep_all_oracle()
    p = sc.keep_all_params(1000)[2]
    assert all(o.idx.size == 1000 for o, pp in zip(orc.rows, p) if pp == 1.0)  # top_k 0 and top_k > V alike
    assert all(o.idx.size < 1000 for o, pp in zip(orc.rows, p) if pp < 1.0)
    assert min(o.top_p_margin for o in orc.rows) > 1e-4
    tail = max(1.0 - o.cdf[sc.LADDER - 1] for o in orc.rows if o.idx.size == 1000)
    assert tail < 1e-6
    for seed in sc.SEEDS:
        for kind in sc.COUNTERS:
            share = orc.band_share(seed, sc.counters(kind))
            print(f"SELECT-COND keep-all seed={seed:#x} counters={kind} band share {share:.4f}, largest tail mass {tail:.2e}")
            assert share <= 0.02 and orc.band_share(seed, sc.counters(kind) + 1) <= 0.02


def test_dyadic_rows_sit_on_the_boundaries():
    orc = sc.dyadic_oracle()
    T, k, p = sc.dyadic_params()
    cnt = sc.dyadic_counters()
    for r, o in enumerate(orc.rows):
        u = sc.draw_u(sc.DYADIC_SEED, int(cnt[r]), r)
        keep = 64 if p[r] == 1.0 else 32
        assert o.idx.size == keep and np.array_equal(o.cdf, np.arange(1, keep + 1) / keep)
        assert np.all(np.diff(o.idx) > 0)  # equal keys: index ascending
        if p[r] == 1.0:
            assert 0 < u < 1 and u * 32 == int(u * 32)
            assert u in o.cdf  # exactly on a partial sum, in fp32 as in fp64: every term is 1.0
        else:
            assert o.top_p_margin == 0.0  # the ascending cumsum of 32 ones is exactly (1 - p) * total
    assert sc.find_boundary_counter(sc.DYADIC_SEED, 8, 1 << 16) == cnt[8]


def _rejected(orc_true: sc.Oracle, orc_bad: sc.Oracle, seed, cnt) -> int:
    acc = orc_true.accepted(seed, cnt)
    bad = orc_bad.expected(seed, cnt)
    return sum(int(bad[r]) not in acc[r] for r in range(len(acc)))


@pytest.mark.parametrize("defect", ["no_row", "counter_plus_1", "neighbour_top_k", "ties_not_extended"])
def test_replay_cases_reject(defect):
    """A kernel that made the mistake would return the mistaken oracle's tokens: count the rows where those
    leave the accepted set, in every replay case the GPU module runs."""
    for V in (1000, 8193):
        good = sc.case_oracle(V)
        bad = sc.Oracle(sc.make_logits(V), *sc.row_params(), defects=(defect,))
        for seed in sc.SEEDS:
            for kind in sc.COUNTERS:
                n = _rejected(good, bad, seed, sc.counters(kind))
                print(f"SELECT-DEFECT {defect} V={V} seed={seed:#x} counters={kind}: {n} rows rejected")
                assert n >= (3 if defect == "ties_not_extended" else 100)


def test_no_row_in_the_hash_means_one_draw_for_a_fresh_batch():
    u = sc.draws(11, sc.counters("zero"), defects=("no_row",))
    assert np.unique(u).size == 1
    assert np.unique(sc.draws(11, sc.counters("zero"))).size == sc.R


def test_only_the_dyadic_rows_decide_the_comparisons():
    good = sc.dyadic_oracle()
    T, k, p = sc.dyadic_params()
    cnt = sc.dyadic_counters()
    want = good.expected(sc.DYADIC_SEED, cnt)
    ge = sc.dyadic_oracle(("pick_ge",)).expected(sc.DYADIC_SEED, cnt)
    lt = sc.dyadic_oracle(("top_p_lt",)).expected(sc.DYADIC_SEED, cnt)
    assert np.all(ge[p == 1.0] != want[p == 1.0])   # every boundary row: the token before
    assert np.all(lt[p == 1.0] == want[p == 1.0])   # no top-p walk on these rows
    assert np.all(lt[p == 0.5] != want[p == 0.5])   # 33 kept for 32
    # the random rows cannot: u is a multiple of 2^-24 and never equals a partial sum of exponentials
    for V in (1000, 8193):
        for defect in ("pick_ge", "top_p_lt"):
            bad = sc.Oracle(sc.make_logits(V), *sc.row_params(), defects=(defect,))
            assert _rejected(sc.case_oracle(V), bad, 11, sc.counters("arange")) == 0


def test_extending_ties_over_neg_inf_changes_no_draw():
    x = np.full(8193, -np.inf, dtype=np.float32)
    x[[17, 4000, 8192]] = [1.0, 0.5, 0.0]
    for p in (1.0, 0.95, 0.5):
        a = sc.row_oracle(x, 1.0, 50, p)
        b = sc.row_oracle(x, 1.0, 50, p, defects=("ties_over_neg_inf",))
        assert a.idx.size <= 3 < b.idx.size or p < 1.0
        for u in np.linspace(0, 1, 257)[:-1]:
            assert sc.pick(a, u) == sc.pick(b, u)


def test_greedy_tie_rows_reject_the_highest_index():
    for n in (2, 64, 1024):
        for spread in (False, True):
            pos = sc.tie_positions(16454, n, spread)
            x = sc.tie_row(16454, pos).numpy()
            assert np.count_nonzero(x == x.max()) == n and pos[0] > 0
            assert (len({int(q) // sc.CHUNK for q in pos}) > 1) == spread
            assert sc.row_oracle(x, 0.0, 50, 1.0).idx[0] == pos[0]
            assert sc.row_oracle(x, 0.0, 50, 1.0, defects=("highest_tied_index",)).idx[0] == pos[-1]


def test_topk_checker_sees_what_it_claims():
    n, k = 32769, 250
    s = sc.topk_scores(n)
    v, i = torch.sort(s, dim=-1, descending=True, stable=True)  # stable: index ascending among equals
    v, i = v[:, :k].contiguous(), i[:, :k].contiguous()
    assert sc.check_topk(v, i, s, k) == []
    assert bool((v[:, 1:] == v[:, :-1]).any())  # ties are plentiful
    j = i.clone()
    tie = int(torch.nonzero(v[0, 1:] == v[0, :-1])[0])
    j[0, [tie, tie + 1]] = j[0, [tie + 1, tie]]
    assert any("ascend" in m for m in sc.check_topk(v, j, s, k))
    j = i.clone()
    j[1, 5] = j[1, 4]
    assert any("repeats" in m or "hold" in m for m in sc.check_topk(v, j, s, k))
    j = i.clone()
    j[2, 0] = -1
    assert any("out of range" in m for m in sc.check_topk(v, j, s, k))
    w = v.clone()
    w[0, -1] = 0.0
    assert sc.check_topk(w, i, s, k)
    # a strictly larger entry left out for a tied one at the k-th value
    s2 = s.clone()
    s2[0, 7] = 2.0
    assert sc.check_topk(v, i, s2, k)


def test_masked_and_ragged_conditions():
    logits, mask, flags, masked, (T, k, p) = sc.masked_case()
    allowed = (masked > float("-inf")).sum(1)
    assert sorted(set(allowed[flags != 0].tolist())) == list(sc.MASK_ALLOWED) and bool((masked[:, -1] > float("-inf")).all())
    assert bool((allowed[flags == 0] == sc.MASK_V).all()) and int((flags == 0).sum()) == sc.MASK_ROWS // 8
    assert int((masked.argmax(1) == sc.MASK_V - 1).sum()) >= sc.MASK_ROWS // 3  # the 1-bit mask word holds the maximum
    cases = [(sc.masked_oracle(), sc.MASK_ROWS)]
    for V, kw in ((8262, {}), (8193, {"single_top_at_end": True})):
        cases.append((sc.Oracle(sc.make_logits(V, rows=128, **kw), *sc.row_params(128)), 128))
    for orc, rows in cases:
        assert min(o.top_p_margin for o in orc.rows) > 1e-4
        for seed in sc.SEEDS:
            for kind in sc.COUNTERS:
                cnt = sc.counters(kind, rows)
                assert orc.band_share(seed, cnt) <= 0.02 and orc.band_share(seed, cnt + 1) <= 0.02
