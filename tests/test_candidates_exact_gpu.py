"""The threshold-candidate kernels of the index search on the exact operands of tests/cand_cases.py: integer
queries and rows, so every score is an exact integer and the candidates of every query are known.  For every
query of every launch, with no tolerance: ``cnt`` is the size of the expected set; the stored indices are that
set, none twice; every stored value is the score of its row bit for bit; nothing is written past
min(cnt, cap), into the guard rows of the lists or into the counts past M.  Queries A and rows B sit in
NaN-guarded buffers with padded strides; behind ``B[:N]``, and in the padding rows of the fragment copy (plus a
spare block), lie rows that would beat every threshold, as do dead rows and rows of other groups.  Each shape is
launched twice: one dense query (every visible row, exactly once: the LDS lists' high-water flush, gemm256's
overflow to direct appends) beside sparse ones with lists that hold everything, and the dense query again with
cap = 64 (``cnt`` keeps counting, the 64 stored entries are distinct members of the set).
tests/test_candidates_exact_cpu.py proves the oracle and shows that the checker rejects each planted mistake.

Kernel instantiation per case, read from ``gemm_score_candidates`` (gemm.hip), the ``score_candidates_shuf``
binding and the launchers (``cand_cases.arm`` mirrors them and is asserted for every case):

    test_index_scan            index_scan_kernel<FMT, MT, NW, 8>, both layouts: M 1 / 16 -> MT 1, 17 / 32 -> MT 2 (NW 4),
                               33 .. 96 -> MT 3 .. 6 (NW 8), a ragged last query tile at 17, 33, 49, 65, 81;
                               K 256, 768 (M 96), 1024 (M 64); N 4, 132 and P + 132 with P = 256 x CUs rows of one
                               grid pass: the VGPR ring crosses a tile boundary and some workgroups run a partial
                               second tile
    test_stream_candidates     stream_gemm ST_EPI_CAND: cfg 7 (row-major, M 32 / 64) and cfg 12 (fragment copy,
                               M 1 / 17 / 64) at K 384; N 4, 132, 4100
    test_gemm_bt_candidates    gemm_bt_kernel<EPI_CANDIDATES, 128, 128, 2, 2, false>: M 1 / 31, K 64 / 320, N 4 / 132 / 1000
    test_gemm_bt_candidates_256_tile   gemm_bt_kernel<EPI_CANDIDATES, 256, 256, 2, 4, false> at 2048 x 5120 x 64: 8 x 20 = 160
                               tiles, the dispatch bound
    test_gemm256_candidates    gemm256_kernel<G_CAND, false, false, SHUF>, both layouts: M 97 / 128 (rows 128-255 of the
                               tile past M: the h2 half-tile skip), 129, 300 (LDS lists), 1025 (past kCandMaxM: the
                               per-tile threshold load and direct appends); K 128 / 384; N 132, 260 and
                               256 x CUs / ceil(M / 256) + 132, where some workgroups take a second tile
    test_dispatch_through_ops  ops.score_candidates / ops.score_candidates_shuffled reach each of the eight arms by shape

No caller can reach: ST_EPI_CAND on cfg 10 (``stream_candidates_launch`` picks it for M > 64 on a fragment
copy, but the binding sends M > 64 with K % 128 == 0 to the scan or to gemm256, and the wrapper refuses other
K); gemm_bt_kernel<EPI_CANDIDATES, ..., SHUF = true> of either tile (a fragment copy with M > 64 always has
K % 128 == 0 and goes to gemm256; M <= 64 goes to the scan or cfg 12); ``gemm256_candidates_stamped`` (a
diagnostic).  They are not tested.

On an MI355X (256 CUs: P = 65,536, the scan's third N is 65,668) all 59 cases pass: every count, set, value and
guard in every launch.  With defects planted one at a time in a scratch build (no address, bound or launch
shape changed; the group lookup clamped to N - 1 where the n < N test was dropped), the tests that failed, and
the 44 tests of tests/test_kernels_gpu.py on candidates, scores and the index that noticed:

    index_scan's hit test ``v > thr``        test_index_scan at every M >= 16 in both layouts (26 cases; M = 1 has no odd
                                             query, and only odd queries sit on an integer threshold) and
                                             test_dispatch_through_ops; earlier tests: none
    gemm256's ``n < p.N`` test dropped       test_gemm256_candidates at M 97 / 128 / 129 / 300, both K, both layouts (16
                                             cases; M = 1025 takes the direct-append arm with its own test) and
                                             test_dispatch_through_ops; earlier tests: none
    the final cand_flush of index_scan       all 28 test_index_scan cases and test_dispatch_through_ops; earlier tests:
    skipped                                  24 (threshold search, exact-set, fragment-layout and recall tests)
"""
import pytest
import torch

import cand_cases as cc
from django_assistant_bot_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAYOUTS = ("rm", "shuf")


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(layout, M, N, K, want_arm):
    got = cc.run(ops, DEV, layout, M, N, K, want_arm)
    assert got == [], (want_arm, layout, M, N, K, got)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,K", cc.SCAN_MK)
def test_index_scan(M, K, layout):
    for N in cc.scan_ns(_cus()):
        _run(layout, M, N, K, f"scan-{layout}")


@pytest.mark.parametrize("layout,M,K", [("rm", m, k) for m, k in cc.STREAM_RM_MK] + [("shuf", m, k) for m, k in cc.STREAM_SHUF_MK])
def test_stream_candidates(layout, M, K):
    for N in cc.STREAM_NS:
        _run(layout, M, N, K, "stream-7" if layout == "rm" else "stream-12")


@pytest.mark.parametrize("M,K", cc.BT_MK)
def test_gemm_bt_candidates(M, K):
    for N in cc.BT_NS:
        _run("rm", M, N, K, "bt128-rm")


def test_gemm_bt_candidates_256_tile():
    M, N, K = cc.BT_BIG
    _run("rm", M, N, K, "bt256-rm")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,K", cc.G256_MK)
def test_gemm256_candidates(M, K, layout):
    for N in cc.g256_ns(M, _cus()):
        _run(layout, M, N, K, f"g256-{layout}")


DISPATCH = (("rm", 17, 132, 256), ("shuf", 17, 132, 256), ("rm", 32, 132, 384), ("shuf", 17, 132, 384),
            ("rm", 31, 132, 320), ("rm", 2048, 5120, 64), ("rm", 129, 260, 128), ("shuf", 129, 260, 128))


def test_dispatch_through_ops():
    """The wrappers own the buffers here, so the guard checks do not apply; everything else does."""
    reached = set()
    for layout, M, N, K in DISPATCH:
        d = cc.data(N, K, 96 if M <= 96 else M)
        thr = cc.thresholds(d, M, dense=True)
        A = d.A[:M].to(torch.bfloat16).to(DEV)
        rg, qg = torch.from_numpy(d.row_group[:N].copy()).to(DEV), torch.from_numpy(d.q_group[:M].copy()).to(DEV)
        t = torch.from_numpy(thr).to(DEV)
        for cap in (N + 8, 64):
            if layout == "rm":
                val, idx, cnt = ops.score_candidates(A, d.B[:N].to(torch.bfloat16).to(DEV), t, cap, rg, qg)
            else:
                R = -(-N // 128) * 128
                full = torch.full((R, K), 2.0, dtype=torch.bfloat16, device=DEV)
                full[:N] = d.B[:N].to(DEV)
                val, idx, cnt = ops.score_candidates_shuffled(A, ops.shuffle_weights(full), N, t, cap, rg, qg)
            torch.cuda.synchronize()
            pad = lambda x: torch.cat([x[:1], x, x[:1]]).cpu()  # noqa: E731  (the checker skips the guard rows)
            res = cc.Result(torch.cat([cnt.cpu(), cnt.new_zeros(cc.CNT_GUARD).cpu()]), pad(val), pad(idx))
            got = cc.check(res, d, M, thr, cap, guards=False)
            assert got == [], (layout, M, N, K, cap, got)
            # the wrapper's own promise: -inf past the count
            stored = cnt.clamp(max=cap)
            assert bool((val[torch.arange(cap, device=DEV)[None, :] >= stored[:, None]] == float("-inf")).all())
        reached.add(cc.arm(layout, M, N, K))
    assert reached == set(cc.ARMS)
