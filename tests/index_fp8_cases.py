"""Cases for the FP8 vector index (``index_scan_kernel<kScanFp8, ...>``, ``index_dequant_kernel``, ``VectorIndex`` with
``dtype=torch.float8_e4m3fn``): the exact operands of tests/cand_cases.py with a per-row power-of-two scale, the
defect emulations of the checker's self-test, and the guarded launch of the FP8 scan.  Pure NumPy / torch-CPU but for
``launch``; tests/test_index_fp8_cpu.py proves the construction, tests/test_index_fp8_gpu.py uses it on the kernels.

Operands: the ``cand_cases`` construction (queries in {0, 1, 2}, rows in {-2 .. 2}, hot / dead rows, groups, anti-hits
behind ``N``) with row n multiplied by 2^(n % 3): row values reach +-8 and the rows get three different exponent
bytes under ``kv_quantize`` (a row whose largest |value| is 2, 4 or 8 is stored as bytes of value 256 x row / 2^i
with exponent byte 120 + i; rows of smaller magnitude differ again).  Every value divided by its row scale is an
integer multiple of 32 up to 256: exact in e4m3fn (3 mantissa bits).  |score| <= 16 K = 16384 < 2^24 at K = 1024, so
every score is an exact integer in fp32 whatever the MFMA order, and the unscaled sums (<= 2 x 256 x K = 2^19) times a
power of two are exact as well: the integer oracle and ``cand_cases.check`` apply unchanged to a ``Data`` built from
the scaled rows.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import cand_cases as cc
from django_assistant_bot_amd.ops import reference as ref

PAD_EXP = 200  # exponent byte of every row past N in the launch's buffers: 2^73, a padding row that scores is a hit


def row_scale(n_rows: int) -> np.ndarray:
    return (2.0 ** (np.arange(n_rows) % 3)).astype(np.float32)


def _base_thr(score: torch.Tensor, visible: torch.Tensor) -> np.ndarray:
    """The thresholds of ``cand_cases.data`` for another score matrix: even queries half below the score of their
    rank-(60 + m % 7) visible row, odd queries on the integer most of their visible rows of ranks 30 .. 66 share."""
    queries = score.shape[0]
    s = torch.where(visible, score, torch.full_like(score, -(1 << 30)))
    ranked = torch.sort(s, dim=1, descending=True).values
    nvis = visible.sum(1)
    base = np.empty(queries, dtype=np.float32)
    for m in range(queries):
        nv = int(nvis[m])
        if nv == 0:
            base[m] = 0.5
            continue
        t = float(ranked[m, min(nv - 1, 60 + m % 7)])
        if m % 2:
            window = ranked[m, min(nv - 1, 30):min(nv, 67)]
            vals, counts = torch.unique(window, return_counts=True)
            t = float(vals[int(torch.argmax(counts))])
        base[m] = t if m % 2 else t - 0.5
    return base


@functools.lru_cache(maxsize=8)
def data(N: int, K: int, queries: int = 96) -> cc.Data:
    """``cand_cases.data(N, K)`` with row n (the rows behind N included) multiplied by 2^(n % 3)."""
    d = cc.data(N, K, queries)
    B = d.B * torch.from_numpy(row_scale(d.B.shape[0]))[:, None]
    score = (d.A.double() @ B[:N].double().t()).to(torch.int32)
    return dataclasses.replace(d, B=B, score=score, base_thr=_base_thr(score, d.visible))


@functools.lru_cache(maxsize=8)
def quantised(N: int, K: int):
    """(bytes uint8 [N, K], exponent bytes uint8 [N]) of the scaled rows; the round trip is asserted exact."""
    d = data(N, K)
    rows = d.B[:N].to(torch.bfloat16)
    q, e = ref.kv_quantize(rows)
    assert torch.equal(ref.kv_dequantize(q, e), d.B[:N])
    return q, e


def unscaled_score(d: cc.Data, swap_halves: bool = False) -> torch.Tensor:
    """int64 [queries, N]: the sums over the stored byte values (what the accumulators hold before the exponent is
    applied).  ``swap_halves``: the two 32-k halves of every 64-k fragment exchanged on the row side."""
    q, _ = ref.kv_quantize(d.B[:d.N].to(torch.bfloat16))
    v = q.view(torch.float8_e4m3fn).double()
    if swap_halves:
        v = v.view(d.N, d.K // 64, 2, 32).flip(2).reshape(d.N, d.K)
    return (d.A.double() @ v.t()).to(torch.int64)


def defective(d: cc.Data, defect: str) -> cc.Data:
    """The ``Data`` whose scores are what a kernel with the planted mistake computes: ``no_exponent`` (the sums are
    compared and stored without the row's 2^(b - 127)), ``swapped_halves`` (the second 32-k half of each 64-k
    fragment meets the queries' first half), ``neighbour_exponent`` (row n is scaled by row n ^ 1's exponent byte)."""
    _, e = ref.kv_quantize(d.B[:d.N].to(torch.bfloat16))
    scale = (e.to(torch.int32) << 23).view(torch.float32).double()
    if defect == "no_exponent":
        s = unscaled_score(d).double()
    elif defect == "swapped_halves":
        s = unscaled_score(d, swap_halves=True).double() * scale[None, :]
    elif defect == "neighbour_exponent":
        nb = torch.arange(d.N) ^ 1
        nb[nb >= d.N] = d.N - 2
        s = unscaled_score(d).double() * scale[nb][None, :]
    else:
        assert defect == "", defect
        s = unscaled_score(d).double() * scale[None, :]
    assert bool((s == s.round()).all()) and float(s.abs().max()) < 2 ** 24
    return dataclasses.replace(d, score=s.to(torch.int32))


def emulate(d: cc.Data, M: int, thr, cap: int, grouped: bool = True, defect: str = "", seed: int = 0) -> cc.Result:
    """What the FP8 scan leaves behind when it computes ``defective(d, defect)``'s scores (hits in any order)."""
    return cc.emulate(defective(d, defect), M, thr, cap, grouped, seed=seed)


def launch(ops, dev, M: int, d: cc.Data, thr: np.ndarray, cap: int, grouped: bool = True) -> cc.Result:
    """The native FP8 launcher on caller-owned, guarded buffers, as ``cand_cases.launch`` does for the bf16 arms: the
    queries in a NaN buffer with a padded stride; the rows quantised into an FP8 fragment copy whose padding rows and
    one spare 128-row block hold hot rows (all 2.0) under the exponent byte ``PAD_EXP``, so a kernel that scores a row
    at n >= N appends it to every list; the exponents behind an 8-byte guard; the lists and counts in sentinel-filled
    memory with guard rows / entries."""
    from django_assistant_bot_amd.ops._lib import ptr, stream

    N, K = d.N, d.K
    nat = ops.native()
    abuf = torch.full((M + 2, K + cc.A_PAD), float("nan"), dtype=torch.bfloat16, device=dev)
    A = abuf[1:M + 1, :K]
    A.copy_(d.A[:M])
    rg = torch.from_numpy(d.row_group).to(dev) if grouped else None
    qg = torch.from_numpy(d.q_group[:M].copy()).to(dev) if grouped else None
    t = torch.from_numpy(thr).to(dev)
    res = cc.empty_result(M, cap)
    cnt, val, idx = res.cnt.to(dev), res.val.to(dev), res.idx.to(dev)
    R = -(-N // 128) * 128 + 128
    q, e = quantised(N, K)
    hot_q, _ = ref.kv_quantize(torch.full((1, K), 2.0, dtype=torch.bfloat16))
    full = hot_q.repeat(R, 1)
    full[:N] = q
    shuf = ops.shuffle_weights_fp8(full.to(dev))
    ebuf = torch.full((8 + R + 8,), PAD_EXP, dtype=torch.uint8, device=dev)
    exps = ebuf[8:8 + R]
    exps[:N] = e.to(dev)
    nat.score_candidates_fp8(ptr(A), A.stride(0), ptr(shuf), ptr(exps), M, N, K, ptr(rg), ptr(qg), ptr(t), ptr(cnt),
                             ptr(val[1]), ptr(idx[1]), cap, stream(A))
    torch.cuda.synchronize()
    assert bool(torch.isnan(abuf[0]).all() and torch.isnan(abuf[-1]).all() and torch.isnan(abuf[:, K:]).all())
    return cc.Result(cnt.cpu(), val.cpu(), idx.cpu())


def run(ops, dev, M: int, N: int, K: int, grouped: bool):
    """The main launch (one dense query beside sparse ones, cap = N + 8: the lists hold every hit) and the overflow
    launch (the dense query again with cap = 64); -> complaints of ``cand_cases.check``."""
    d = data(N, K)
    out = []
    thr = cc.thresholds(d, M, dense=M > 1)
    cap = N + 8
    out += [f"main: {c}" for c in cc.check(launch(ops, dev, M, d, thr, cap, grouped), d, M, thr, cap, grouped)]
    thr = cc.thresholds(d, M, dense=True)
    out += [f"cap 64: {c}" for c in cc.check(launch(ops, dev, M, d, thr, 64, grouped), d, M, thr, 64, grouped)]
    return out
