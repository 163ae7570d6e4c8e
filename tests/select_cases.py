"""Cases and CPU oracle for the selection kernels of select.hip (``sample_tokens``, ``sample_candidates`` ->
``sample_merge``, ``mask_logits``, ``topk_rows``).  Pure Python / NumPy / torch-CPU; the GPU module
(tests/test_select_exact_gpu.py) and the CPU module that proves the oracle (tests/test_select_exact_cpu.py)
share everything here.

The draw of a row is a pure function of (seed, counter, row, logits, T, k, p):

    u = (splitmix64(seed ^ splitmix64(counter * 0x9E3779B97F4A7C15 + row)) >> 40) / 2^24      (64-bit wrap-around)

so a test can replay it: HF semantics in fp64 (temperature -> top-k keeping every logit equal to the k-th,
never over -inf, at most 1024 kept -> the ascending-cumsum top-p rule that keeps at least one -> the CDF over
the kept set in (key descending, index ascending) order) give the one token a row must return, except where
``u`` lies within DELTA of a CDF boundary, where either side of that boundary passes.

DELTA = 2^-14 in u-space: ``__expf``, the divide and a <= 64-term fp32 sum put each cumulative probability
within about 2^-17 relative; 2^-14 leaves 8 x over that.

``defects`` names a planted mistake that the oracle then makes on purpose; the CPU module shows which case
rejects each.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

DELTA = 2.0 ** -14
CAP = 1024           # SEL_MAXK: the most tokens the one-pass sampler keeps
CHUNK = 256 * 32     # tokens per chunk_topk_kernel workgroup
R = 512
VOCABS = (1000, 8192, 8193, 16454, 131072)
PATHS = ("exact", "fast", "tp2", "tp8")
SEEDS = (11, 0xDEADBEEFCAFEF00D)
COUNTERS = ("zero", "arange", "big")
TEMPS = (0.0, 0.7, 1.0, 1.3)
TOP_KS = (1, 3, 50, 64)
TOP_PS = (0.5, 0.95, 1.0)
LADDER = 60
DEFECTS = ("no_row", "counter_plus_1", "pick_ge", "top_p_lt", "ties_not_extended", "ties_over_neg_inf",
           "neighbour_top_k", "highest_tied_index")

_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------------------------------------
# keys and the counter RNG


def float_key(f) -> np.ndarray:
    """Order-preserving uint32 key of fp32 values (common.h ``float_key``)."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_float(k) -> np.ndarray:
    k = np.ascontiguousarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def splitmix64(x: int) -> int:
    x = (x + _GOLD) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def draw_u(seed: int, counter: int, row: int) -> float:
    """The uniform of (seed, counter, row): a multiple of 2^-24 in [0, 1), exact in fp32 and fp64."""
    inner = splitmix64(((counter & _M64) * _GOLD + row) & _M64)
    return (splitmix64((seed & _M64) ^ inner) >> 40) / 16777216.0


def draws(seed: int, counters, defects=()) -> np.ndarray:
    out = np.empty(len(counters))
    for r, c in enumerate(counters):
        c = int(c) + (1 if "counter_plus_1" in defects else 0)
        out[r] = draw_u(seed, c, 0 if "no_row" in defects else r)
    return out


def counters(kind: str, rows: int = R) -> np.ndarray:
    """Counters that collide across rows: only ``row`` in the hash keeps such rows apart."""
    if kind == "zero":
        return np.zeros(rows, dtype=np.int64)
    if kind == "arange":
        return np.arange(rows, dtype=np.int64)
    assert kind == "big"
    c = np.full(rows, 7, dtype=np.int64)
    c[rows // 3] = (1 << 32) + 5  # the product with the odd constant wraps past 2^64
    c[rows // 2] = (1 << 62) + 1
    return c


# ---------------------------------------------------------------------------------------------
# rows


def row_params(rows: int = R):
    """Every (T, top_k, top_p) combination, a different one on neighbouring rows."""
    r = np.arange(rows)
    T = np.array(TEMPS, dtype=np.float32)[r % 4]
    k = np.array(TOP_KS, dtype=np.int32)[(r // 4 + r) % 4]
    p = np.array(TOP_PS, dtype=np.float32)[(r // 16 + r) % 3]
    return T, k, p


def ladder_values(kind: int) -> np.ndarray:
    """60 values 0.125 apart from 12.0 down (exact in bf16).  kind 1: ranks 47..52 share a value (top-k 50
    keeps 53); kind 2: ranks 2 and 3 share one (top-k 3 keeps 4)."""
    v = 12.0 - 0.125 * np.arange(LADDER, dtype=np.float32)
    if kind == 1:
        v[47:53] = v[47]
    elif kind == 2:
        v[2:4] = v[2]
    return v


@functools.lru_cache(maxsize=None)
def make_logits(V: int, rows: int = R, seed: int = 0, steep: bool = False, single_top_at_end: bool = False):
    """fp32 [rows, V], every value exact in bf16.  Each row: its own permutation of the ladder at its own
    positions, spread over the chunks; 40 distinct background values 2.0, 1.9375, ... below it (so top-k 64
    reaches four of them, untied); the rest of the background on a 1/32 grid in [-8, -1].  ``steep``: the
    whole background on a 1/8 grid in [-24, -16], so that rows which keep everything (top_k 0 or > V) put
    under 1e-6 of their mass in the tail.  ``single_top_at_end``: every third row (greedy and sampled ones alike) has its maximum at V - 1."""
    rng = np.random.default_rng(1000 * V + seed)
    if steep:
        x = -16.0 - rng.integers(0, 65, size=(rows, V)).astype(np.float32) / 8.0
    else:
        x = -1.0 - rng.integers(0, 225, size=(rows, V)).astype(np.float32) / 32.0
    nbg = 0 if steep else 40
    bg = 2.0 - 0.0625 * np.arange(nbg, dtype=np.float32)
    for r in range(rows):
        vals = np.concatenate([rng.permutation(ladder_values(r % 5)), bg])
        pos = rng.choice(V - 1 if single_top_at_end else V, len(vals), replace=False)  # uniform over the chunks
        x[r, pos] = vals
        if single_top_at_end and r % 3 == 0:
            x[r, V - 1] = 12.5
    t = torch.from_numpy(x)
    assert torch.equal(t.to(torch.bfloat16).float(), t)
    return t


# ---------------------------------------------------------------------------------------------
# the oracle


@dataclasses.dataclass
class RowOracle:
    idx: np.ndarray      # kept tokens in CDF order (key descending, index ascending); one entry when greedy
    cdf: np.ndarray      # cumulative probability after each kept token, cdf[-1] == 1; empty when greedy
    top_p_margin: float  # smallest |prefix sum - (1 - p) total| / ((1 - p) total) of the top-p walk (inf if none)

    @property
    def greedy(self) -> bool:
        return self.cdf.size == 0


def _sorted_top(x: np.ndarray, m: int):
    """Indices of the m largest entries, (value descending, index ascending)."""
    m = min(m, x.size)
    if m < x.size:
        part = np.argpartition(-x, m - 1)[:m]
        kth = x[part].min()
        part = np.nonzero(x >= kth)[0]  # all of the ties at the cut, so that the index order is exact
    else:
        part = np.arange(x.size)
    order = np.lexsort((part, -x[part].astype(np.float64)))
    return part[order]


def row_oracle(x: np.ndarray, T: float, k: int, p: float, cap: int = CAP, default_k: int = CAP, defects=()) -> RowOracle:
    """x: one row of logits (fp32 values).  ``default_k``: what top_k <= 0 means (1024 in the one-pass
    kernel, 64 in the merge)."""
    V = x.size
    if T <= 0:
        top = x.max()
        tied = np.nonzero(x == top)[0]
        pick = tied[-1] if "highest_tied_index" in defects else tied[0]
        return RowOracle(np.array([pick]), np.empty(0), np.inf)
    k = min(k if k > 0 else default_k, default_k, cap, V)
    order = _sorted_top(x, max(k, cap) + 1)
    xs = x[order].astype(np.float64)
    kth = xs[k - 1]
    if "ties_not_extended" in defects:
        n = k
    else:
        n = int(np.searchsorted(-xs, -kth, side="right"))  # every logit equal to the k-th stays
    if "ties_over_neg_inf" not in defects:
        n = min(n, int(np.count_nonzero(xs > -np.inf)))    # ... but never a -inf one
    n = max(1, min(n, cap))
    order, xs = order[:n], xs[:n]
    z = xs / np.float64(np.float32(T))
    e = np.exp(z - z[0])
    total = e.sum()
    keep, margin = n, np.inf
    if p < 1.0:
        thr = (1.0 - np.float64(np.float32(p))) * total
        cum = np.cumsum(e[::-1])[: n - 1]            # ascending: the smallest first, the largest never dropped
        drop = (cum < thr) if "top_p_lt" in defects else (cum <= thr)
        ndrop = int(np.argmin(drop)) if not drop.all() else drop.size  # the walk stops at the first survivor
        keep = n - ndrop
        if cum.size:
            margin = float(np.min(np.abs(cum - thr)) / thr)
    cdf = np.cumsum(e[:keep])
    cdf /= cdf[-1]
    return RowOracle(order[:keep], cdf, margin)


def pick(o: RowOracle, u: float, defects=()) -> int:
    """The kernel's walk: the first token whose cumulative probability exceeds u."""
    if o.greedy:
        return int(o.idx[0])
    side = "left" if "pick_ge" in defects else "right"
    i = int(np.searchsorted(o.cdf, u, side=side))
    return int(o.idx[min(i, o.idx.size - 1)])


def accepted(o: RowOracle, u: float, delta: float = DELTA) -> set:
    """Tokens that pass: the oracle's, and where u is within delta of a CDF boundary, that boundary's
    other neighbour."""
    if o.greedy:
        return {int(o.idx[0])}
    lo = int(np.searchsorted(o.cdf, u - delta, side="right"))
    hi = int(np.searchsorted(o.cdf, u + delta, side="right"))
    last = o.idx.size - 1
    return {int(t) for t in o.idx[min(lo, last): min(hi, last) + 1]}


def boundary_distance(o: RowOracle, u: float) -> float:
    """|u - the nearest interior CDF boundary| (inf for a row with one kept token)."""
    if o.greedy or o.idx.size < 2:
        return np.inf
    return float(np.min(np.abs(o.cdf[:-1] - u)))


class Oracle:
    """Per-row oracles of one launch: logits [rows, V] with per-row T / top_k / top_p."""

    def __init__(self, logits: torch.Tensor, T, k, p, default_k: int = CAP, defects=()):
        x = logits.float().numpy()
        self.defects = tuple(defects)
        kk = np.roll(k, 1) if "neighbour_top_k" in self.defects else k
        self.rows = [row_oracle(x[r], float(T[r]), int(kk[r]), float(p[r]), default_k=default_k, defects=self.defects)
                     for r in range(x.shape[0])]
        self.sampled = np.array([not o.greedy for o in self.rows])

    def expected(self, seed: int, cnt) -> np.ndarray:
        u = draws(seed, cnt, self.defects)
        return np.array([pick(o, u[r], self.defects) for r, o in enumerate(self.rows)])

    def accepted(self, seed: int, cnt):
        u = draws(seed, cnt)
        return [accepted(o, u[r]) for r, o in enumerate(self.rows)]

    def band_share(self, seed: int, cnt) -> float:
        return float(np.mean([len(a) > 1 for a in self.accepted(seed, cnt)]))

    def distances(self, seed: int, cnt) -> np.ndarray:
        u = draws(seed, cnt)
        return np.array([boundary_distance(o, u[r]) for r, o in enumerate(self.rows)])


@functools.lru_cache(maxsize=None)
def case_oracle(V: int, default_k: int = CAP) -> Oracle:
    return Oracle(make_logits(V), *row_params(), default_k=default_k)


def keep_all_params(V: int, rows: int = R):
    """top_k 0 and top_k > V on alternating rows (both keep min(V, 1024) tokens), sampled rows only."""
    r = np.arange(rows)
    T = np.array((0.7, 1.0, 1.3), dtype=np.float32)[r % 3]
    k = np.where(r % 2 == 0, 0, V + 1 + r).astype(np.int32)
    p = np.array(TOP_PS, dtype=np.float32)[(r // 3) % 3]
    return T, k, p


@functools.lru_cache(maxsize=None)
def keep_all_oracle(V: int = 1000) -> Oracle:
    return Oracle(make_logits(V, steep=True), *keep_all_params(V))


# The comparisons themselves (``acc > target``, ``cum <= thr``) are decided only where both sides are equal,
# which a random row never gives.  A row of 64 tied maxima does: every exp() is 1.0, every partial sum a small
# integer, top_p 0.5 puts the ascending cumsum exactly on (1 - p) * total after 32 tokens, and a counter
# chosen so that u = j / 32 or j / 64 puts the target exactly on a partial sum -- in fp32 as in fp64, so these
# rows are replayed with no DELTA at all.
DYADIC_V = 16454
DYADIC_ROWS = 16
DYADIC_SEED = 5


def _splitmix64_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(_GOLD)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def draws_np(seed: int, cnt: np.ndarray, row: int) -> np.ndarray:
    """``draw_u`` for many counters of one row at once."""
    with np.errstate(over="ignore"):
        inner = _splitmix64_np(cnt.astype(np.uint64) * np.uint64(_GOLD) + np.uint64(row))
        return (_splitmix64_np(np.uint64(seed & _M64) ^ inner) >> np.uint64(40)).astype(np.float64) / 16777216.0


def dyadic_params(rows: int = DYADIC_ROWS):
    r = np.arange(rows)
    T = np.ones(rows, dtype=np.float32)
    k = np.full(rows, 64, dtype=np.int32)
    p = np.where(r % 2 == 0, 1.0, 0.5).astype(np.float32)
    return T, k, p


@functools.lru_cache(maxsize=None)
def dyadic_logits() -> torch.Tensor:
    x = make_logits(DYADIC_V, rows=DYADIC_ROWS, seed=3).clone()
    rng = np.random.default_rng(99)
    for r in range(DYADIC_ROWS):
        x[r, torch.from_numpy(rng.choice(DYADIC_V, 64, replace=False))] = 13.0  # above the ladder: exactly 64 kept
    return x


def find_boundary_counter(seed: int, row: int, span: int = 1 << 23) -> int:
    """The first counter of ``row`` whose u is an interior multiple of 1/32 (a boundary of both CDFs)."""
    u = draws_np(seed, np.arange(span, dtype=np.uint64), row) * 32.0
    return int(np.nonzero((u == np.floor(u)) & (u > 0))[0][0])


# find_boundary_counter(DYADIC_SEED, row) for rows 0..15 (a search of seconds: kept as constants, and
# verified draw by draw in the CPU module)
_BOUNDARY_COUNTERS = (300321, 289329, 341711, 334172, 483929, 1087668, 1437543, 1121817, 44705, 1091248,
                      1001520, 297444, 121833, 156169, 2017623, 356055)


def _off_boundary_counter(seed: int, row: int) -> int:
    """The first counter whose u picks another token among 33 equal ones than among 32, well inside both."""
    for c in range(1000):
        u = draw_u(seed, c, row)
        if int(33 * u) != int(32 * u) and 0.1 < (33 * u) % 1 < 0.9 and 0.1 < (32 * u) % 1 < 0.9:
            return c
    raise AssertionError("no such counter")


def dyadic_counters() -> np.ndarray:
    """Even rows (top_p 1.0, 64 kept): u exactly on a partial sum, which decides ``acc > target``.  Odd rows
    (top_p 0.5): the cumsum of the 32 smallest is exactly (1 - p) * total, which decides ``cum <= thr``: 32 are
    kept, and u is one that draws another token if 33 are."""
    return np.array([_BOUNDARY_COUNTERS[r] if r % 2 == 0 else _off_boundary_counter(DYADIC_SEED, r)
                     for r in range(DYADIC_ROWS)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def dyadic_oracle(defects=()) -> Oracle:
    return Oracle(dyadic_logits(), *dyadic_params(), defects=defects)


def check_replay(tokens, oracle: Oracle, seed: int, cnt):
    """-> (rows whose token is not accepted, share of rows in the DELTA band, the largest |u - boundary|
    among rows whose token differs from the oracle's)."""
    tokens = np.asarray(tokens)
    acc = oracle.accepted(seed, cnt)
    want = oracle.expected(seed, cnt)
    bad = [r for r in range(len(acc)) if int(tokens[r]) not in acc[r]]
    dist = oracle.distances(seed, cnt)
    differ = tokens != want
    worst = float(dist[differ].max()) if differ.any() else 0.0
    return bad, float(np.mean([len(a) > 1 for a in acc])), worst


def slices(V: int, tp: int):
    """Vocabulary slices of a TP group: widths that are no multiple of 8 wherever V / tp is not one
    (1000 / 8 = 125, 8193 / 2 = 4096.5, 16454 / 8 = 2056.75), offsets that leave bf16 rows unaligned."""
    b = [round(V * i / tp) for i in range(tp + 1)]
    return list(zip(b[:-1], b[1:]))


def draw(ops, path: str, logits, T, k, p, seed: int, cnt):
    """One launch on the GPU through ``path``; ``cnt`` is advanced in place."""
    V = logits.shape[1]
    if path in ("exact", "fast"):
        return ops.sample_tokens(logits, T, k, p, seed, cnt, fast=(path == "fast"))
    tp = int(path[2:])
    parts = [ops.sample_candidates(logits[:, a:b], b - a, a) for a, b in slices(V, tp)]
    return ops.sample_merge(torch.cat(parts, 2).contiguous(), T, k, p, seed, cnt, V)


# ---------------------------------------------------------------------------------------------
# masked rows


MASK_V = 8193
MASK_ROWS = 96
MASK_ALLOWED = (1, 3, 70)


@functools.lru_cache(maxsize=None)
def masked_case():
    """-> (logits fp32 [rows, V], mask int32 [rows, 257], row_flags int32 [rows], masked logits, (T, k, p)).
    Rows with 1, 3 and 70 allowed tokens under top_k 50 (fewer allowed than k; more allowed than k), token
    8192 -- the one valid bit of the last mask word -- always among them, and its logit the row's largest
    allowed one on every other row; every eighth row is unflagged and must stay as it is."""
    V, rows = MASK_V, MASK_ROWS
    logits = make_logits(V, rows=rows, seed=5).clone()
    logits[::2, V - 1] = 12.5
    rng = np.random.default_rng(21)
    words = -(-V // 32)
    bits = np.zeros((rows, words * 32), dtype=bool)
    flags = np.ones(rows, dtype=np.int32)
    for r in range(rows):
        n = MASK_ALLOWED[r % 3]
        top = np.argsort(-logits[r].numpy(), kind="stable")[:40]
        pool = np.concatenate([rng.choice(top, min(n - 1, 20), replace=False), rng.choice(V - 1, n, replace=False)])
        allowed = np.concatenate([[V - 1], rng.permutation(np.setdiff1d(np.unique(pool), [V - 1]))[: n - 1]])
        bits[r, allowed] = True
        if r % 8 == 7:
            flags[r] = 0
    bits[:, V:] = rng.integers(0, 2, size=(rows, words * 32 - V)).astype(bool)  # bits past the vocabulary: ignored
    w = (bits.reshape(rows, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    mask = torch.from_numpy(w.view(np.int32).copy())
    allow = torch.from_numpy(bits[:, :V] | (flags == 0)[:, None])
    masked = logits.masked_fill(~allow, float("-inf"))
    r = np.arange(rows)
    T = np.array((0.7, 1.0, 0.0, 1.3), dtype=np.float32)[(r // 3) % 4]
    k = np.full(rows, 50, dtype=np.int32)
    p = np.array(TOP_PS, dtype=np.float32)[(r // 12) % 3]
    return logits, mask, torch.from_numpy(flags), masked, (T, k, p)


@functools.lru_cache(maxsize=None)
def masked_oracle() -> Oracle:
    return Oracle(masked_case()[3], *masked_case()[4])


# ---------------------------------------------------------------------------------------------
# greedy ties


def tie_row(V: int, positions) -> torch.Tensor:
    x = make_logits(V, rows=1, seed=7)[0].clone()
    x[torch.as_tensor(positions)] = 12.25
    return x


def tie_positions(V: int, n: int, spread: bool, seed: int = 0):
    """n tied maxima: inside the last full chunk, or spread over every chunk; never index 0."""
    rng = np.random.default_rng(n + 17 * seed + (1 if spread else 0))
    if spread:
        return np.sort(1 + rng.choice(V - 1, n, replace=False))
    lo = (V // CHUNK - 1) * CHUNK
    return np.sort(lo + 1 + rng.choice(CHUNK - 1, n, replace=False))


# ---------------------------------------------------------------------------------------------
# topk_rows


TOPK_NS = (1024, 32767, 32768, 32769, 32768 + 100)
TOPK_KS = (1, 63, 64, 65, 250, 1024)
TOPK_ROWS = 3
TOPK_BASE = (1 << 33) + 5


@functools.lru_cache(maxsize=None)
def topk_scores(n: int, rows: int = TOPK_ROWS) -> torch.Tensor:
    """fp32 scores on a grid of 2^-10 steps in [-1, 1]: exact, with about n / 2049 entries per value."""
    g = torch.Generator().manual_seed(n)
    return torch.randint(-1024, 1025, (rows, n), generator=g).float() / 1024.0


def check_topk(vals, idx, scores: torch.Tensor, k: int, valid=None):
    """``scores`` [rows, n] on the CPU (what the kernel read); ``valid`` [rows]: entries past it are -inf
    padding of the caller.  Returns a list of complaints (empty: the result is a correct top-k)."""
    vals, idx = vals.cpu(), idx.cpu().long()
    want = torch.topk(scores, k, dim=-1).values
    out = []
    if not torch.equal(vals, want):
        out.append("values differ from torch.topk")
    for r in range(scores.shape[0]):
        i, v, s = idx[r], vals[r], scores[r]
        if int(i.min()) < 0 or int(i.max()) >= s.numel():
            out.append(f"row {r}: index out of range ({int(i.min())}, {int(i.max())})")
            continue
        if not torch.equal(s[i], v):
            out.append(f"row {r}: an index does not hold its value")
        if i.unique().numel() != k:
            out.append(f"row {r}: an index repeats")
        same = v[1:] == v[:-1]
        if bool((same & (i[1:] <= i[:-1])).any()):
            out.append(f"row {r}: indices among equal values do not ascend")
        above = set(torch.nonzero(s > want[r, -1]).flatten().tolist())
        if not above <= set(i.tolist()):
            out.append(f"row {r}: an index above the k-th value is missing")
        if valid is not None and int(valid[r]) >= k and int(i.max()) >= int(valid[r]):
            out.append(f"row {r}: an index from the padding")
    return out
