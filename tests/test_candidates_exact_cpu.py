"""The oracle and the checker of tests/cand_cases.py, proved on the CPU: the integer expected sets against
``ops.reference.gemm_bt(EPI_SCORES)`` plus a threshold, the properties the cases rely on (exact scores, rows
that score exactly the integer thresholds, hot rows that beat every threshold), and that ``check`` accepts
what a correct kernel may leave behind -- hits in any order -- and rejects each planted mistake in the case
built for it:

    > for >=                          the odd queries: rows whose score is the threshold are missing
    no n < N test                     the hot rows behind B[:N] / in the padding of the fragment copy surface
    the group filter ignoring -1      the queries with q_group = -1 come back empty
    a dropped flush                   a wave's last list never arrives: count and set fall short
    a repeated flush                  it arrives twice: the count is too high and indices repeat
"""
import numpy as np
import pytest
import torch

import cand_cases as cc
from django_assistant_bot_amd.ops import reference as ref

SHAPES = [(4, 256), (132, 256), (1000, 64), (4100, 384)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_expected_sets_match_the_reference_scores(N, K):
    d = cc.data(N, K)
    M = 33
    thr = cc.thresholds(d, M, dense=True)
    A, B = d.A[:M].to(torch.bfloat16), d.B[:N].to(torch.bfloat16)
    assert torch.equal(A.float(), d.A[:M]) and torch.equal(B.float(), d.B[:N])
    assert int(d.score.abs().max()) <= 4 * K < 2 ** 24
    for grouped in (True, False):
        s = ref.gemm_bt(A, B, epilogue=ref.EPI_SCORES, out_f32=True,
                        row_group=torch.from_numpy(d.row_group[:N]) if grouped else None,
                        q_group=torch.from_numpy(d.q_group[:M].copy()) if grouped else None)
        want = s >= torch.from_numpy(thr)[:, None]
        assert torch.equal(want, cc.expected(d, M, thr, grouped))
        finite = torch.isfinite(s)
        assert torch.equal(s[finite], d.score[:M].float()[finite])


@pytest.mark.parametrize("N,K", SHAPES[1:])
def test_cases_hold_what_they_promise(N, K):
    d = cc.data(N, K)
    M = 96
    thr = cc.thresholds(d, M, dense=True)
    want = cc.expected(d, M, thr)
    at_thr = (d.score[:M].float() == torch.from_numpy(thr)[:, None]) & d.visible[:M]
    odd = np.arange(M - 1) % 2 == 1
    assert bool((at_thr.sum(1)[:M - 1][odd] >= 1).all())       # every integer threshold is some row's score
    assert N < 1000 or bool((at_thr.sum(1)[:M - 1][odd] >= 2).all())  # ... and of several
    assert int(at_thr.sum(1)[:M - 1][~odd].sum()) == 0          # the half-integer ones are nobody's
    assert torch.equal(want[M - 1], d.visible[M - 1])           # the dense query: every visible row
    hot = torch.from_numpy(d.hot)
    assert bool(want[:, hot][d.visible[:M][:, hot]].all())      # a hot row is a hit wherever it is visible
    assert d.hot[0] and d.hot[N - 1] and d.hot[(N - 1) // 16 * 16] and d.hot[5]
    sparse = want[:M - 1].sum(1)
    assert int(sparse.max()) <= 120 and int(sparse.min()) >= 1
    assert set(d.q_group[:M].tolist()) == {-1, 0, 1, 2} and (d.row_group[:N] < 0).any()
    assert bool((d.B[N:] == 2).all()) and (d.row_group[N:] >= 0).all()


@pytest.mark.parametrize("cap", [None, 64])
@pytest.mark.parametrize("grouped", [True, False])
def test_checker_accepts_any_order_and_rejects_each_planted_mistake(grouped, cap):
    d = cc.data(1000, 64)
    M = 31
    thr = cc.thresholds(d, M, dense=True)
    cap = cap or d.N + 8
    for seed in (0, 1):
        assert cc.check(cc.emulate(d, M, thr, cap, grouped, seed=seed), d, M, thr, cap, grouped) == []
    reasons = {"gt": "cnt differs", "no_n_bound": "cnt differs", "dropped_flush": "cnt differs",
               "repeated_flush": "cnt differs", "minus_one_matches_nothing": "cnt differs"}
    for defect, first in reasons.items():
        if defect == "minus_one_matches_nothing" and not grouped:
            continue
        got = cc.check(cc.emulate(d, M, thr, cap, grouped, defect=defect), d, M, thr, cap, grouped)
        assert got and first in got[0], (defect, got)
        text = " | ".join(got)
        if cap > 64:
            if defect == "no_n_bound":
                assert "out of range" in text
            if defect == "repeated_flush":
                assert "repeats" in text
            if defect in ("gt", "dropped_flush", "minus_one_matches_nothing"):
                assert "missing or extra" in text
    # the counts alone are not the whole check: right counts over wrong entries
    res = cc.emulate(d, M, thr, cap, grouped)
    res.idx[1, 0] = res.idx[1, 1]
    assert any("repeats" in c for c in cc.check(res, d, M, thr, cap, grouped))
    res = cc.emulate(d, M, thr, cap, grouped)
    res.val[3, 0] += 1.0
    assert any("not the score" in c for c in cc.check(res, d, M, thr, cap, grouped))
    res = cc.emulate(d, M, thr, cap, grouped)
    res.cnt[M] = 0
    res.val[2, int(res.cnt[1].clamp(max=cap)):] = 0.0
    got = " | ".join(cc.check(res, d, M, thr, cap, grouped))
    assert "past M" in got and ("past min(cnt, cap)" in got or int(res.cnt[1]) >= cap)
    res = cc.emulate(d, M, thr, cap, grouped)
    res.idx[-1, 3] = 7
    assert any("guard row" in c for c in cc.check(res, d, M, thr, cap, grouped))


def test_which_rows_decide_each_mistake():
    d = cc.data(1000, 64)
    M = 31
    thr = cc.thresholds(d, M, dense=True)
    want = cc.expected(d, M, thr)
    gt = cc.expected(d, M, thr, defect="gt")
    lost = (want & ~gt).sum(1).numpy()
    m = np.arange(M)
    assert (lost[(m % 2 == 1) & (m < M - 1)] >= 1).all() and (lost[m % 2 == 0] == 0).all()
    none = cc.expected(d, M, thr, defect="minus_one_matches_nothing").sum(1).numpy()
    assert (none[d.q_group[:M] < 0] == 0).all() and (want.sum(1).numpy()[d.q_group[:M] < 0] > 0).all()
    assert np.array_equal(none[d.q_group[:M] >= 0], want.sum(1).numpy()[d.q_group[:M] >= 0])


def test_every_arm_is_named_by_some_case():
    cus = 256
    reached = set()
    for M, K in cc.SCAN_MK:
        for N in cc.scan_ns(cus):
            reached |= {cc.arm("rm", M, N, K), cc.arm("shuf", M, N, K)}
    for M, K in cc.STREAM_RM_MK:
        reached.add(cc.arm("rm", M, 132, K))
    for M, K in cc.STREAM_SHUF_MK:
        reached.add(cc.arm("shuf", M, 132, K))
    for M, K in cc.BT_MK:
        reached.add(cc.arm("rm", M, 132, K))
    reached.add(cc.arm("rm", *cc.BT_BIG[:2], cc.BT_BIG[2]))
    for M, K in cc.G256_MK:
        for N in cc.g256_ns(M, cus):
            reached |= {cc.arm("rm", M, N, K), cc.arm("shuf", M, N, K)}
    assert reached == set(cc.ARMS)
    assert cc.scan_pass_rows(cus) == (8 // 4) * cus * 32 * 4 == (8 // 8) * cus * 32 * 8
    # the last N of gemm256 gives some workgroups a second tile; the 256-tile of gemm.hip sits on its bound
    for M, _ in cc.G256_MK:
        assert -(-M // 256) * -(-cc.g256_ns(M, cus)[2] // 256) > cus
    assert -(-cc.BT_BIG[0] // 256) * -(-cc.BT_BIG[1] // 256) == 160
    # a fragment copy never reaches gemm.hip's candidate epilogue: M > 64 with K % 128 == 0 is gemm256's
    assert all(cc.arm("shuf", M, 132, K) != "bt128-rm" for M in (1, 64, 65, 97, 300) for K in (128, 384, 1280))
