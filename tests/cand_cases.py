"""Cases and CPU oracle for the threshold-candidate kernels of the index search (``index_scan_kernel``,
``stream_gemm`` with the candidate epilogue, ``gemm_bt_kernel<EPI_CANDIDATES>``, ``gemm256_kernel<G_CAND>``) on
exact operands.  Pure NumPy / torch-CPU but for ``launch``, which the GPU module (tests/test_candidates_exact_gpu.py)
calls; tests/test_candidates_exact_cpu.py proves the oracle and the checker.

Operands: queries A in {0, 1, 2}, index rows B in {-2 .. 2}, as bf16.  |score| <= 4 K = 4096 < 2^24 at the
largest K used (1024), so every score is an exact integer in fp32 whatever the MFMA order, and the expected set
of every query is computed in integers on the CPU.  A *hot* row is all 2: it scores 2 * sum(A[m]), the largest
score any row can have against any query, so it is a hit of every query that may see it -- and an anti-hit
wherever it must not be seen: behind ``B[:N]`` in the parent buffer and in the padding rows of the fragment
copy (n >= N), with ``row_group`` < 0 (dead), and in another group than the query's.

Thresholds: even queries sit half below the score of their rank-(60 + m % 7) visible row (nothing is near); odd
queries on the integer that most of their visible rows of ranks 30 .. 66 share (those rows decide ``>=``).
One query of the launch is dense: its threshold is below every score, so every visible row must appear
exactly once.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

VAL_SENTINEL = -777.0
IDX_SENTINEL = -555
CNT_SENTINEL = 12345
A_PAD = B_PAD = 8
CNT_GUARD = 8
DENSE_THR = -1.0e9

# (M, K) of every arm, read from gemm_score_candidates / the score_candidates_shuf binding / the launchers
SCAN_MK = tuple((m, 256) for m in (1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96)) + ((96, 768), (64, 1024))
STREAM_RM_MK = ((32, 384), (64, 384))          # cfg 7
STREAM_SHUF_MK = ((1, 384), (17, 384), (64, 384))  # cfg 12
STREAM_NS = (4, 132, 4100)
BT_MK = ((1, 64), (31, 64), (1, 320), (31, 320))
BT_NS = (4, 132, 1000)
BT_BIG = (2048, 5120, 64)
G256_MK = tuple((m, k) for m in (97, 128, 129, 300, 1025) for k in (128, 384))


def scan_pass_rows(cus: int) -> int:
    """Rows one full grid pass of index_scan covers: (8 / NW) workgroups per CU x 32 NW rows each."""
    return 256 * cus


def scan_ns(cus: int):
    return (4, 132, scan_pass_rows(cus) + 132)


def g256_ns(M: int, cus: int):
    return (132, 260, 256 * (cus // -(-M // 256)) + 132)


def arm(layout: str, M: int, N: int, K: int) -> str:
    """The kernel a call reaches (gemm.hip ``gemm_score_candidates``, bindings.cpp ``score_candidates_shuf``)."""
    scan = K % 256 == 0 and ((M <= 64 and K <= 1024) or (M <= 96 and K <= 768))
    if layout == "shuf":
        assert K % 128 == 0  # ops.score_candidates_shuffled refuses anything else
        if scan:
            return "scan-shuf"
        return "stream-12" if M <= 64 else "g256-shuf"  # M > 64 and K % 128 == 0: always gemm256, never gemm.hip
    if K % 128 == 0 and (M >= 128 or (M > 64 and not scan)):
        return "g256-rm"
    if scan:
        return "scan-rm"
    if 32 <= M <= 64 and K % 128 == 0:
        return "stream-7"
    big = M >= 2048 and N >= 512 and -(-M // 256) * -(-N // 256) >= 160
    return "bt256-rm" if big else "bt128-rm"


ARMS = ("scan-rm", "scan-shuf", "stream-7", "stream-12", "bt128-rm", "bt256-rm", "g256-rm", "g256-shuf")


def _round_up(x: int, m: int) -> int:
    return -(-x // m) * m


@dataclasses.dataclass
class Data:
    """Operands of one (N, K), shared by every M: the first M queries are the case's."""
    N: int
    K: int
    A: torch.Tensor          # [queries, K] fp32 integers
    B: torch.Tensor          # [N + behind, K] fp32 integers: rows N.. are hot (the anti-hits behind B[:N])
    hot: np.ndarray          # bool [N]
    row_group: np.ndarray    # int32 [N + behind] (-1 dead; rows behind N are live and in every group's way)
    q_group: np.ndarray      # int32 [queries]
    score: torch.Tensor      # int32 [queries, N]
    visible: torch.Tensor    # bool [queries, N]
    base_thr: np.ndarray     # fp32 [queries]


@functools.lru_cache(maxsize=8)
def data(N: int, K: int, queries: int = 96) -> Data:
    rng = np.random.default_rng(7919 * N + K)
    behind = _round_up(N, 256) + 32 - N
    A = rng.integers(0, 3, size=(queries, K)).astype(np.float32)
    B = rng.integers(-2, 3, size=(N + behind, K)).astype(np.float32)
    hot = np.zeros(N, dtype=bool)
    r = np.arange(N)
    hot[[0, N - 1]] = True
    hot[(r >= N - 512) & np.isin(r % 16, (0, 15))] = True   # first and last row of the 16-row blocks of the last tiles
    hot[(r < 256) & (r % 32 == 5)] = True                     # one in each wave's slice of the first workgroup tile
    hot[rng.random(N) < 0.004] = True
    B[:N][hot] = 2.0
    B[N:] = 2.0
    row_group = rng.integers(0, 3, size=N + behind).astype(np.int32)
    row_group[rng.random(N + behind) < 0.2] = -1
    row_group[N:] = np.arange(behind) % 3  # live, of every group: only n < N keeps them out
    if N >= 4:
        row_group[0], row_group[N - 1] = 0, 1
    q = np.arange(queries)
    q_group = np.where(q % 4 == 3, -1, q % 3).astype(np.int32)
    At, Bt = torch.from_numpy(A), torch.from_numpy(B)
    score = (At.double() @ Bt[:N].double().t()).to(torch.int32)
    rg = torch.from_numpy(row_group[:N]).long()[None, :]
    qg = torch.from_numpy(q_group).long()[:, None]
    visible = (rg >= 0) & ((qg < 0) | (rg == qg))
    s = torch.where(visible, score, torch.full_like(score, -(1 << 30)))
    ranked = torch.sort(s, dim=1, descending=True).values
    nvis = visible.sum(1)
    base = np.empty(queries, dtype=np.float32)
    for m in range(queries):
        if int(nvis[m]) == 0:
            base[m] = 0.5
            continue
        nv = int(nvis[m])
        t = float(ranked[m, min(nv - 1, 60 + m % 7)])
        if m % 2:  # the integer kind: the most shared score among ranks 30 .. 66
            window = ranked[m, min(nv - 1, 30):min(nv, 67)]
            vals, counts = torch.unique(window, return_counts=True)
            t = float(vals[int(torch.argmax(counts))])
        base[m] = t if m % 2 else t - 0.5
    return Data(N, K, At, Bt, hot, row_group, q_group, score, visible, base)


def thresholds(d: Data, M: int, dense: bool) -> np.ndarray:
    thr = d.base_thr[:M].copy()
    if dense:
        thr[M - 1] = DENSE_THR
    return thr


def expected(d: Data, M: int, thr: np.ndarray, grouped: bool = True, defect: str = "") -> torch.Tensor:
    """bool [M, N]: the candidates of every query.  ``defect``: a planted mistake of the filter."""
    t = torch.from_numpy(thr.astype(np.float64))[:, None]
    s = d.score[:M].double()
    hit = (s > t) if defect == "gt" else (s >= t)
    if grouped:
        vis = d.visible[:M]
        if defect == "minus_one_matches_nothing":
            rg = torch.from_numpy(d.row_group[:d.N]).long()[None, :]
            vis = (rg >= 0) & (rg == torch.from_numpy(d.q_group[:M]).long()[:, None])
        hit = hit & vis
    return hit


# ---------------------------------------------------------------------------------------------
# results and the checker


@dataclasses.dataclass
class Result:
    cnt: torch.Tensor       # int32 [M + CNT_GUARD]
    val: torch.Tensor       # fp32 [M + 2, cap] (guard rows first and last)
    idx: torch.Tensor       # int32 [M + 2, cap]


def empty_result(M: int, cap: int) -> Result:
    cnt = torch.full((M + CNT_GUARD,), CNT_SENTINEL, dtype=torch.int32)
    cnt[:M] = 0
    return Result(cnt, torch.full((M + 2, cap), VAL_SENTINEL), torch.full((M + 2, cap), IDX_SENTINEL, dtype=torch.int32))


def emulate(d: Data, M: int, thr, cap: int, grouped: bool = True, defect: str = "", seed: int = 0) -> Result:
    """What a correct kernel may leave behind (hits in an arbitrary order), or one with a planted mistake:
    ``gt`` / ``minus_one_matches_nothing`` (see ``expected``), ``no_n_bound`` (the hot rows behind B[:N] score and
    are appended), ``dropped_flush`` (one wave's last list of up to 96 hits never reaches the global lists),
    ``repeated_flush`` (it reaches them twice)."""
    rng = np.random.default_rng(seed)
    want = expected(d, M, thr, grouped, defect)
    res = empty_result(M, cap)
    for m in range(M):
        n = torch.nonzero(want[m]).flatten().numpy()
        v = d.score[m].numpy()[n].astype(np.float32)
        if defect == "no_n_bound":
            extra = np.arange(d.N, d.B.shape[0])
            ok = np.ones(extra.size, bool)
            if grouped:
                rg = d.row_group[extra]
                ok = (rg >= 0) & ((d.q_group[m] < 0) | (rg == d.q_group[m]))
            n = np.concatenate([n, extra[ok]])
            v = np.concatenate([v, np.full(int(ok.sum()), 2.0 * float(d.A[m].sum()), dtype=np.float32)])
        order = rng.permutation(n.size)
        n, v = n[order], v[order]
        if defect == "dropped_flush" and n.size:
            keep = n.size - min(96, max(1, n.size // 3))
            n, v = n[:keep], v[:keep]
        if defect == "repeated_flush" and n.size:
            rep = min(96, max(1, n.size // 3))
            n, v = np.concatenate([n, n[-rep:]]), np.concatenate([v, v[-rep:]])
        res.cnt[m] = n.size
        w = min(n.size, cap)
        res.val[m + 1, :w] = torch.from_numpy(v[:w])
        res.idx[m + 1, :w] = torch.from_numpy(n[:w].astype(np.int32))
    return res


def check(res: Result, d: Data, M: int, thr, cap: int, grouped: bool = True, guards: bool = True):
    """Every query, no excuses.  -> list of complaints (empty: the result is right)."""
    out = []
    want = expected(d, M, thr, grouped)
    cnt = res.cnt[:M].long()
    if not torch.equal(cnt, want.sum(1)):
        bad = torch.nonzero(cnt != want.sum(1)).flatten()[:4].tolist()
        out.append(f"cnt differs at queries {bad}: got {cnt[bad].tolist()}, want {want.sum(1)[bad].tolist()}")
    stored = cnt.clamp(max=cap)
    val, idx = res.val[1:M + 1], res.idx[1:M + 1].long()
    col = torch.arange(cap)[None, :]
    live = col < stored[:, None]
    if guards:
        if not bool((res.cnt[M:] == CNT_SENTINEL).all()):
            out.append("a count past M was touched")
        if not bool(((val == VAL_SENTINEL) & (idx == IDX_SENTINEL))[~live].all()):
            out.append("an entry past min(cnt, cap) was written")
        for g in (0, -1):
            if not bool((res.val[g] == VAL_SENTINEL).all() and (res.idx[g] == IDX_SENTINEL).all()):
                out.append("a guard row of the lists was written")
    rows = torch.arange(M)[:, None].expand(M, cap)[live]
    n = idx[live]
    if n.numel() and (int(n.min()) < 0 or int(n.max()) >= d.N):
        out.append(f"index out of range: {int(n.min())} .. {int(n.max())} (N = {d.N})")
        return out
    seen = torch.zeros((M, d.N), dtype=torch.int32)
    seen.index_put_((rows, n), torch.ones_like(n, dtype=torch.int32), accumulate=True)
    if int(seen.max()) > 1 if seen.numel() else False:
        out.append("an index repeats within a query")
    if bool(((seen > 0) & ~want).any()):
        m, r = torch.nonzero((seen > 0) & ~want)[0].tolist()
        out.append(f"query {m} holds row {r}, which is no candidate (score {int(d.score[m, r])}, thr {float(thr[m])})")
    full = cnt <= cap
    if bool((((seen > 0) != want) & full[:, None]).any()):
        m, r = torch.nonzero(((seen > 0) != want) & full[:, None])[0].tolist()
        out.append(f"query {m}: row {r} missing or extra (score {int(d.score[m, r])}, thr {float(thr[m])})")
    if not torch.equal(val[live], d.score[:M][rows, n].float()):
        out.append("a stored value is not the score of its row")
    return out


# ---------------------------------------------------------------------------------------------
# the launch (GPU)


def launch(ops, dev, layout: str, M: int, d: Data, thr: np.ndarray, cap: int, grouped: bool = True,
           spare_block: bool = True) -> Result:
    """The native launcher on caller-owned, guarded buffers: A in a NaN buffer with a padded stride; B row-major
    likewise with the hot rows behind N and NaN after them, or a fragment copy whose padding rows (and one
    spare 128-row block) are hot; the lists and counts in sentinel-filled memory with guard rows / entries."""
    from django_assistant_bot_amd.ops._lib import ptr, stream

    N, K = d.N, d.K
    nat = ops.native()
    abuf = torch.full((M + 2, K + A_PAD), float("nan"), dtype=torch.bfloat16, device=dev)
    A = abuf[1:M + 1, :K]
    A.copy_(d.A[:M])
    rg = torch.from_numpy(d.row_group).to(dev) if grouped else None
    qg = torch.from_numpy(d.q_group[:M].copy()).to(dev) if grouped else None
    t = torch.from_numpy(thr).to(dev)
    res = empty_result(M, cap)
    cnt, val, idx = res.cnt.to(dev), res.val.to(dev), res.idx.to(dev)
    args = (ptr(rg), ptr(qg), ptr(t), ptr(cnt), ptr(val[1]), ptr(idx[1]), cap, stream(A))
    if layout == "rm":
        rows = d.B.shape[0]
        bbuf = torch.full((rows + 16, K + B_PAD), float("nan"), dtype=torch.bfloat16, device=dev)
        bbuf[:rows, :K] = d.B.to(dev)
        nat.gemm_score_candidates(ptr(A), A.stride(0), ptr(bbuf), bbuf.stride(0), M, N, K, *args)
    else:
        R = _round_up(N, 128) + (128 if spare_block else 0)
        full = torch.full((R, K), 2.0, dtype=torch.bfloat16, device=dev)
        full[:N] = d.B[:N].to(dev)
        shuf = ops.shuffle_weights(full)
        nat.score_candidates_shuf(ptr(A), A.stride(0), ptr(shuf), M, N, K, *args, R)
    torch.cuda.synchronize()
    assert bool(torch.isnan(abuf[0]).all() and torch.isnan(abuf[-1]).all() and torch.isnan(abuf[:, K:]).all())
    return Result(cnt.cpu(), val.cpu(), idx.cpu())


def run(ops, dev, layout: str, M: int, N: int, K: int, want_arm: str, overflow: bool = True):
    """The main launch (one dense query beside sparse ones, lists that hold every hit) and the overflow launch
    (the dense query again with cap = 64); -> complaints."""
    assert arm(layout, M, N, K) == want_arm, (layout, M, N, K, arm(layout, M, N, K))
    d = data(N, K, 96 if M <= 96 else M)
    out = []
    thr = thresholds(d, M, dense=M > 1)
    cap = N + 8
    out += [f"main: {c}" for c in check(launch(ops, dev, layout, M, d, thr, cap), d, M, thr, cap)]
    if overflow:
        thr = thresholds(d, M, dense=True)
        out += [f"cap 64: {c}" for c in check(launch(ops, dev, layout, M, d, thr, 64), d, M, thr, 64)]
    return out
