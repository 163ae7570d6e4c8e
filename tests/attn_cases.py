"""Attention inputs in which a single key is visible, and the checkers that read them.

Random q / k / v make the attention output an average of many values: one dropped, leaked or
misplaced key moves a row by less than a bf16 rounding, so no tolerance can see it.  The inputs
built here make single keys decisive instead:

* **Position-coded V.**  Every cache slot / packed row holds a bf16-exact code of (position, kv head,
  sequence): 14 + 4 + 4 sign bits, then a fixed +1 / -1 / 0 pattern, 32 dims in all, tiled over D.
  Two different slots differ by 2.0 in at least one dim, and a wrong output names the slot it
  came from (``decode_code``).
* **Needles.**  A needle row's q is a row of a +-1 Hadamard matrix (times a per-head factor >= 1,
  shared direction inside a GQA group); the key at the chosen position j is parallel to it with a
  scaled score of >= 30 nats.  Background K is 0.1 * randn (scores within about +-0.6), the needle
  directions of one sequence are mutually orthogonal (other needles score exactly 0), and background
  q rows are projected off every needle direction.  The foreign softmax weight of a needle row is
  below N * e^(0.6 - 30) (2e-9 at N = 8192): its output must be the code of slot j, to one bf16
  rounding of 1.0 (2^-8) -- a wrong, missing or extra key moves some dim by >= 1.
* **Anti-needles.**  Keys that must NOT be visible carry the q direction at twice the needle score
  and the code of another slot: the key at causal position p + 1, the unused tail of each
  sequence's last KV block, a spare "stale" block every block-table padding column points at, and in
  packed batches the last key of the previous / first key of the next sequence (sequences alternate
  between two direction sets, so a sequence's own edge keys are orthogonal to its own rows).  A leak
  flips the needle row to the wrong code; everything stays finite.
* **Relative check** on the other rows against a full fp64 reference: per (row, head)
  ``|out - ref| <= tau |ref|`` (2-norms), ``tau = 4 f`` (at most 1.5e-2), where ``f`` is the largest
  such ratio of a bf16 emulation of the same reference (fp64 scores, P = exp(S - rowmax) rounded to
  bf16 in the numerator, an unrounded row sum as the kernels keep it, O rounded to bf16).

Everything is plain torch, built on the CPU from a seeded generator and moved to the device.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import torch

POS_BITS, HEAD_BITS, SEQ_BITS = 14, 4, 4
PATTERN = (1, -1, 0, 1, -1, 0, 1, -1, 0, 1)
STALE_SEQ = 15  # sequence field of the stale block's codes (no case has 16 sequences)
NDIR = 8  # needle rows per sequence: directions 8 * (seq % 2) + r of the Hadamard matrix
NEEDLE_NATS = 30.0
HEAD_FACTORS = (1.0, 1.25, 1.5)
NEEDLE_TOL = 2.0 ** -8
TAU_FACTOR, TAU_CAP = 4.0, 1.5e-2
BG_K = 0.1
SEAMS = (31, 32, 63, 64, 127, 128)


def code(pos, head, seq, D):
    """[..., D] fp32 code of broadcastable integer tensors (position, kv head, sequence)."""
    pos, head, seq = torch.broadcast_tensors(torch.as_tensor(pos), torch.as_tensor(head), torch.as_tensor(seq))
    bits = torch.cat([(pos[..., None] >> torch.arange(POS_BITS)) & 1, (head[..., None] >> torch.arange(HEAD_BITS)) & 1,
                      (seq[..., None] >> torch.arange(SEQ_BITS)) & 1], -1)
    pat = torch.tensor(PATTERN, dtype=torch.float32).expand(*bits.shape[:-1], len(PATTERN))
    c = torch.cat([2.0 * bits.float() - 1.0, pat], -1)
    return c.repeat(*([1] * (c.dim() - 1)), D // c.shape[-1])


def decode_code(vec):
    """(position, kv head, sequence) a (near-)code vector names; for failure messages."""
    b = (vec[:POS_BITS + HEAD_BITS + SEQ_BITS].float().cpu() > 0).long()
    val = lambda x: int((x << torch.arange(x.numel())).sum())  # noqa: E731
    return val(b[:POS_BITS]), val(b[POS_BITS:POS_BITS + HEAD_BITS]), val(b[POS_BITS + HEAD_BITS:])


def hadamard(D):
    H = torch.ones(1, 1)
    while H.shape[0] < D:
        H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
    return H


def needle_coef(scale, D, nats=NEEDLE_NATS):
    """|k| entries of a needle key: nats / (scale D) rounded up to 4 significant bits, so that the
    sums of needle and anti-needle contributions stay bf16-exact."""
    m, e = math.frexp(nats / (scale * D))
    return math.ldexp(math.ceil(m * 16) / 16, e)


@dataclass(eq=False)
class Case:
    kind: str  # "decode" | "paged" | "packed"
    q: torch.Tensor  # [T, Hq, D] (decode: T = B)
    k: torch.Tensor  # cache [blocks, Hkv, bs, D] or packed [Tk, Hkv, D]
    v: torch.Tensor
    qlens: list
    klens: list
    causal: bool
    scale: float
    bt: torch.Tensor | None = None  # int32 [B, cols]; padding columns hold the stale block's index
    bs: int = 0
    part: int = 512
    # needle rows: global q row, sequence, absolute position of the row, key position per kv head,
    # the expected output [R, Hq, D]
    n_row: torch.Tensor = None
    n_seq: torch.Tensor = None
    n_pos: torch.Tensor = None
    n_key: torch.Tensor = None
    n_exp: torch.Tensor = None
    _cache: dict = field(default_factory=dict)

    @property
    def device(self):
        return self.q.device

    @property
    def Hq(self):
        return self.q.shape[1]

    @property
    def Hkv(self):
        return self.k.shape[1]

    @property
    def D(self):
        return self.q.shape[2]

    @property
    def B(self):
        return len(self.klens)

    def cu(self, lens):
        return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=self.device)

    @property
    def cu_q(self):
        return self.cu(self.qlens)

    @property
    def cu_k(self):
        return self.cu(self.klens)

    @property
    def ctx(self):
        return torch.tensor(self.klens, dtype=torch.int32, device=self.device)

    def to(self, device):
        if torch.device(device) == self.device:
            return self
        mv = lambda t: None if t is None else t.to(device)  # noqa: E731
        return Case(self.kind, mv(self.q), mv(self.k), mv(self.v), self.qlens, self.klens, self.causal, self.scale,
                    mv(self.bt), self.bs, self.part, mv(self.n_row), mv(self.n_seq), mv(self.n_pos), mv(self.n_key),
                    mv(self.n_exp))


def decode_positions(c, bs, part):
    """The keys a decode needle may sit on at context c: both ends, the 32-key sub-tile, 128-key,
    block and partition seams, the first slot of the last partition and of the last block."""
    cand = [0, c - 1, c - 2, bs - 1, bs, 31, 32, 127, 128, part - 1, part, (c - 1) // part * part,
            (c - 1) // bs * bs]
    return list(dict.fromkeys(x for x in cand if 0 <= x < c))


def prefill_rows(m, seams=SEAMS):
    """Needle rows of an m-row query chunk: first, last and the rows at the query-block seams."""
    rows = list(dict.fromkeys(i for i in (0, m - 1) + tuple(seams) if 0 <= i < m))
    assert len(rows) <= NDIR
    return rows


def prefill_keys(p, n, causal, first=()):
    """The keys a prefill / packed needle of a row at position p may sit on (``first``: a case's own
    seams, tried before the common ones)."""
    cand = list(first) + [p, 0, n - 1, 63, 64, 31, 32, 127, 128]
    return list(dict.fromkeys(j for j in cand if 0 <= j < n and (j <= p or not causal)))


def _build(kind, klens, qlens, Hq, Hkv, D, bs, causal, scale, seed, needles, shift, seams, part, pad_cols, own_keys=()):
    g = torch.Generator().manual_seed(seed)
    G = Hq // Hkv
    B = len(klens)
    assert B < STALE_SEQ and Hkv <= 1 << HEAD_BITS and max(klens) <= 1 << POS_BITS
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    H = hadamard(D)
    c30 = needle_coef(scale, D)
    dsum = [H[:NDIR].sum(0), H[NDIR:2 * NDIR].sum(0)]
    fac = torch.tensor([HEAD_FACTORS[i % len(HEAD_FACTORS)] for i in range(G)]).repeat(Hkv)  # [Hq]
    paged = kind != "packed"

    # background q, orthogonal to every needle direction
    T = sum(qlens)
    q = torch.randn(T, Hq, D, generator=g)
    q = q - (q @ H[:2 * NDIR].t()) @ H[:2 * NDIR] / D

    Ks, Vs, n_row, n_seq, n_pos, n_key = [], [], [], [], [], []
    q0, counter = 0, shift
    for b, (n, m) in enumerate(zip(klens, qlens)):
        n_alloc = -(-n // bs) * bs if paged else n
        pos = torch.arange(n_alloc)
        K = (BG_K if needles else 1.0) * torch.randn(n_alloc, Hkv, D, generator=g)
        C = torch.zeros(n_alloc, Hkv, D)
        M = torch.zeros(n_alloc, Hkv, dtype=torch.bool)
        par = b % 2
        if needles:
            if kind == "decode":
                rows = [0]
            else:
                rows = prefill_rows(m, seams)
            for r, i in enumerate(rows):
                p = n - m + i
                keys, dirs = [], []
                for hk in range(Hkv):
                    if kind == "decode":
                        cand = decode_positions(n, bs, part)
                        keys.append(cand[counter % len(cand)])
                        dirs.append(NDIR * par + hk % NDIR)
                        counter += 1
                    else:
                        cand = prefill_keys(p, n, causal, own_keys)
                        keys.append(cand[(r + hk + shift) % len(cand)])
                        dirs.append(NDIR * par + r)
                for hk, (j, d) in enumerate(zip(keys, dirs)):
                    C[j, hk] += c30 * H[d]
                    M[j, hk] = True
                    q[q0 + i, hk * G:(hk + 1) * G] = fac[hk * G:(hk + 1) * G, None] * H[d]
                    if causal and p + 1 < n:  # the key just past the diagonal
                        C[p + 1, hk] += 2 * c30 * H[d]
                        M[p + 1, hk] = True
                n_row.append(q0 + i)
                n_seq.append(b)
                n_pos.append(p)
                n_key.append(keys)
        if paged:  # the unused tail of the last block: every direction, at the anti-needle score
            C[n:] = 2 * c30 * (dsum[0] + dsum[1])
            M[n:] = True
        else:  # the neighbours' rows must not see this sequence's edge keys
            edge = torch.zeros(n, dtype=torch.bool)
            edge[0] |= b > 0
            edge[n - 1] |= b < B - 1
            C[edge] += 2 * c30 * dsum[1 - par]
            M[edge] = True
        Ks.append(torch.where(M[..., None], C, K))
        Vc = code(pos[:, None], torch.arange(Hkv)[None, :], b, D)
        if not needles:  # random values (codes only where no key may be read)
            Vc[:n] = torch.randn(n, Hkv, D, generator=g)
        Vs.append(Vc)
        q0 += m

    case = dict(qlens=list(qlens), klens=list(klens), causal=causal, scale=scale, part=part)
    bf = lambda t: t.to(torch.bfloat16)  # noqa: E731
    if paged:
        nblk = [-(-n // bs) for n in klens]
        total = sum(nblk)
        perm = torch.randperm(total + 1, generator=g)
        stale = int(perm[total])
        kc = torch.empty(total + 1, Hkv, bs, D)
        vc = torch.empty(total + 1, Hkv, bs, D)
        kc[stale] = 2 * c30 * (dsum[0] + dsum[1])
        vc[stale] = code(torch.arange(bs)[None, :], torch.arange(Hkv)[:, None], STALE_SEQ, D)
        bt = torch.full((B, max(nblk) + pad_cols), stale, dtype=torch.int32)
        o = 0
        for b, nb in enumerate(nblk):
            idx = perm[o:o + nb]
            bt[b, :nb] = idx.to(torch.int32)
            kc[idx] = Ks[b].view(nb, bs, Hkv, D).permute(0, 2, 1, 3)
            vc[idx] = Vs[b].view(nb, bs, Hkv, D).permute(0, 2, 1, 3)
            o += nb
        case.update(k=bf(kc), v=bf(vc), bt=bt, bs=bs)
    else:
        case.update(k=bf(torch.cat(Ks)), v=bf(torch.cat(Vs)))
    if n_row:
        key = torch.tensor(n_key)  # [R, Hkv]
        seq = torch.tensor(n_seq)
        exp = code(key, torch.arange(Hkv)[None, :], seq[:, None], D).repeat_interleave(G, dim=1)
        case.update(n_row=torch.tensor(n_row), n_seq=seq, n_pos=torch.tensor(n_pos), n_key=key, n_exp=exp)
    return Case(kind=kind, q=bf(q), **case)


def decode_case(ctx, Hq, Hkv, D=128, bs=64, part=512, scale=None, seed=0, needles=True, shift=0, pad_cols=0):
    """One query per sequence; one needle per (sequence, kv head), walking ``decode_positions``."""
    return _build("decode", ctx, [1] * len(ctx), Hq, Hkv, D, bs, False, scale, seed, needles, shift, SEAMS, part,
                  pad_cols)


def paged_case(ctx, qlens, Hq, Hkv, D=128, bs=64, causal=True, scale=None, seed=0, needles=True, shift=0,
               seams=SEAMS, pad_cols=1, keys=()):
    """Query chunks that are the tails of paged contexts; needle rows of ``prefill_rows``."""
    return _build("paged", ctx, qlens, Hq, Hkv, D, bs, causal, scale, seed, needles, shift, seams, 512, pad_cols, keys)


def packed_case(klens, Hq, Hkv, D, causal, qlens=None, scale=None, seed=0, needles=True, shift=0, seams=SEAMS):
    """Packed sequences; ``qlens`` (default: klens) makes q the last rows of each sequence."""
    return _build("packed", klens, klens if qlens is None else qlens, Hq, Hkv, D, 1, causal, scale, seed, needles,
                  shift, seams, 512, 0)


# ------------------------------------------------------------------------------------------------
# the cases (shared by the CPU self-test and the GPU tests)

_A = dict(ctx=[8192, 2049, 513, 65], Hq=32, Hkv=8)
_B_CTX = [1100, 1, 63, 64, 65, 512, 513, 127, 129]
_F = dict(ctx=[300, 200, 65, 129], qlens=[300, 70, 1, 129], Hq=8, Hkv=2)
_G = dict(ctx=[130, 300, 200, 257, 320, 131, 192, 255], qlens=[130, 260, 200, 257, 256, 131, 192, 255], Hq=32, Hkv=8,
          seams=(63, 64, 127, 128, 255, 256))
_G2 = dict(ctx=[520, 194, 257, 1, 64, 485, 33, 129, 301, 5, 513], qlens=[520, 130, 257, 1, 64, 385, 33, 129, 300, 5, 513],
           Hq=64, Hkv=8, seams=(127, 128, 255, 256, 383, 384))
_GODD = dict(ctx=[260, 130, 321, 1, 64, 200, 33, 129, 256, 5, 138], qlens=[260, 130, 257, 1, 64, 200, 33, 129, 256, 5, 131],
             Hq=12, Hkv=4, seams=(63, 64, 127, 128, 255, 256))
_LONG = dict(ctx=[8300, 4200], qlens=[70, 40], Hq=8, Hkv=2, keys=(4095, 4096, 8191, 8192))
_LENS = [1, 63, 64, 65, 127, 128, 129, 5]
_SHORT = [1, 63, 64, 33, 17, 64, 5, 32]
_QTAIL = [1, 20, 64, 33, 100, 128, 70, 5]

CASES = {
    # decode a: the two-slot LDS-DMA kernel (batch * Hkv = 32 <= 64), 16 partitions of 512 when split
    "dec_a-s0": lambda **kw: decode_case(**_A, **kw),
    "dec_a-s8": lambda **kw: decode_case(**_A, shift=8, seed=1, **kw),
    "dec_a-scale": lambda **kw: decode_case(**_A, shift=4, seed=2, scale=0.11, **kw),
    # decode b: batch * Hkv = 72 > 64, the one-slot LDS-DMA kernel
    "dec_b-p512": lambda **kw: decode_case(_B_CTX, 32, 8, part=512, seed=3, **kw),
    "dec_b-p2048": lambda **kw: decode_case(_B_CTX, 32, 8, part=2048, seed=4, shift=5, **kw),
    # decode c: D 64, the register-staged kernel
    **{f"dec_c-s{s}": (lambda s=s, **kw: decode_case([700, 65, 1], 8, 2, D=64, seed=5 + s, shift=s, **kw))
       for s in (0, 4, 8)},
    # decode d: 32- and 128-slot blocks under the 32-key sub-tiles (d, e: 3 partitions of 128 when split)
    **{f"dec_d-bs{bs}-s{s}": (lambda bs=bs, s=s, **kw: decode_case([300, 129], 8, 2, bs=bs, part=128, seed=20 + s, shift=s,
                                                                    **kw))
       for bs in (32, 128) for s in (0, 4, 8)},
    # decode e: GQA groups of 16 (the whole MFMA N dimension) and 2 (14 padded columns)
    **{f"dec_e-g16-s{s}": (lambda s=s, **kw: decode_case([300, 65, 1], 16, 1, part=128, seed=30 + s, shift=s, **kw))
       for s in (0, 3, 6, 9)},
    **{f"dec_e-g2-s{s}": (lambda s=s, **kw: decode_case([300, 65, 1], 4, 2, part=128, seed=40 + s, shift=s, **kw))
       for s in (0, 4, 8)},
    # paged prefill f / h: pair_wgs = 2 * 8 * 4 = 64 < 256, one query block per workgroup
    **{f"pre_f-{'c' if c else 'n'}": (lambda c=c, **kw: paged_case(**_F, causal=c, seed=50, **kw)) for c in (True, False)},
    **{f"pre_h-d{D}-{'c' if c else 'n'}": (lambda D=D, c=c, **kw: paged_case(**_F, D=D, causal=c, seed=51, shift=1, **kw))
       for D in (64, 32) for c in (True, False)},
    # paged prefill g: 3 query blocks -> 2 pairs * 32 heads * 8 sequences = 512 >= 256: paired
    "pre_g": lambda **kw: paged_case(**_G, causal=True, seed=52, **kw),
    # 3 pairs * 64 heads * 11 sequences = 2112 >= 2048: two pairs per workgroup (5 blocks: pairs (4, 0), (3, 1) in
    # the first group, the middle block alone in the second); the grid follows the longest chunk alone
    "pre_g2": lambda **kw: paged_case(**_G2, causal=True, seed=53, **kw),
    # 2 pairs * 12 heads * 11 sequences = 264 >= 256 with (Hq * batch) % 8 = 4: paired, XCD-major walk (no lpt)
    "pre_g-odd": lambda **kw: paged_case(**_GODD, causal=True, seed=54, **kw),
    # flash_d128 keeps the block ids of key tiles 0-63 and 64-127 in two registers and reads later ones from
    # memory: needles on both sides of keys 4096 and 8192 (chunked prefill at the end of long contexts)
    "pre_long": lambda **kw: paged_case(**_LONG, causal=True, seed=55, **kw),
    # packed: D 32 / 64 the encoder kernel; D 128 wide (max_seqlen_q 129 > 64) and narrow
    **{f"pack-d{D}": (lambda D=D, **kw: packed_case(_LENS, 4, 4, D, False, seed=60, **kw)) for D in (32, 64)},
    **{f"pack-d128-{'c' if c else 'n'}": (lambda c=c, **kw: packed_case(_LENS, 8, 2, 128, c, seed=61, **kw))
       for c in (True, False)},
    **{f"pack-d128-short-{'c' if c else 'n'}": (lambda c=c, **kw: packed_case(_SHORT, 8, 2, 128, c, seed=62, shift=2, **kw))
       for c in (True, False)},
    **{f"pack-qtail-{'c' if c else 'n'}": (lambda c=c, **kw: packed_case(_LENS, 8, 2, 128, c, qlens=_QTAIL, seed=63, **kw))
       for c in (True, False)},
}


@functools.lru_cache(maxsize=None)
def get_case(name, device="cpu", needles=True):
    """The named case on ``device``, built once per process (with its reference cached on it).
    ``needles=False``: the same geometry and stale data with background rows only, unit-variance
    K and random V, so that every row (all of a decode case's rows are needle rows) takes the
    relative check on a signal that shrinks with the context as real attention outputs do."""
    return CASES[name](needles=needles).to(device)


# ------------------------------------------------------------------------------------------------
# references


def logical_kv(case, b, n=None, left=0, right=0):
    """K, V [n', Hkv, D] of sequence b: its first ``n`` (default: all valid) keys; paged ``n`` may
    run past the context into the block tail and the padding columns, packed ``left`` / ``right``
    extend the row range into the neighbours."""
    n = case.klens[b] if n is None else n
    if case.kind == "packed":
        s = sum(case.klens[:b])
        sl = slice(s - left, s + n + right)
        return case.k[sl], case.v[sl]
    nb = -(-n // case.bs)
    blocks = case.bt[b, :nb].long()
    gather = lambda c: c[blocks].permute(0, 2, 1, 3).reshape(nb * case.bs, case.Hkv, case.D)[:n]  # noqa: E731
    return gather(case.k), gather(case.v)


def attend(case, b, K, V, dtype=torch.float64, visible=None, emulate=False):
    """Attention of sequence b's query rows over K / V [n, Hkv, D] in ``dtype``.  ``visible`` [m, n]
    bool replaces the case's own mask (all keys, or causal with the rows as the tail of the n keys)."""
    G = case.Hq // case.Hkv
    q0 = sum(case.qlens[:b])
    m, n = case.qlens[b], K.shape[0]
    q = case.q[q0:q0 + m].to(dtype)
    s = torch.einsum("qhd,khd->hqk", q, K.to(dtype).repeat_interleave(G, dim=1)) * case.scale
    if visible is None and case.causal:
        visible = causal_mask(case, b, n)
    if visible is not None:
        s = s.masked_fill(~visible[None], float("-inf"))
    Vd = V.to(dtype).repeat_interleave(G, dim=1)
    if not emulate:
        return torch.einsum("hqk,khd->qhd", s.softmax(-1), Vd)
    p = (s - s.amax(-1, keepdim=True)).exp()
    pb = p.float().to(torch.bfloat16).to(dtype)
    o = torch.einsum("hqk,khd->qhd", pb, Vd) / p.sum(-1).t()[..., None]
    return o.float().to(torch.bfloat16).to(dtype)


def causal_mask(case, b, n, shift=0, strict=False):
    """[m, n] visibility of key j to the row at position p = klen - m + i: j <= p + shift (j < p + shift
    when ``strict``)."""
    m = case.qlens[b]
    p = torch.arange(m, device=case.device)[:, None] + (case.klens[b] - m) + shift
    j = torch.arange(n, device=case.device)[None, :]
    return j < p if strict else j <= p


def reference(case):
    """(ref64 [T, Hq, D], bf16 emulation of it) -- computed once per case."""
    if "ref" not in case._cache:
        outs = [[], []]
        for b in range(case.B):
            K, V = logical_kv(case, b)
            for o, emu in zip(outs, (False, True)):
                o.append(attend(case, b, K, V, emulate=emu))
        case._cache["ref"] = tuple(torch.cat(o) for o in outs)
    return case._cache["ref"]


def rel_err(x, ref):
    """Per (row, head) |x - ref|_2 / |ref|_2."""
    return (x.double() - ref).norm(dim=-1) / ref.norm(dim=-1)


def emulation_floor(case):
    """f: the largest relative error of the bf16 emulation over the non-needle rows (None when
    every row is a needle row)."""
    if "f" not in case._cache:
        ref, emu = reference(case)
        r = rel_err(emu, ref)[plain_rows(case)]
        case._cache["f"] = float(r.max()) if r.numel() else None
    return case._cache["f"]


def plain_rows(case):
    keep = torch.ones(case.q.shape[0], dtype=torch.bool, device=case.device)
    if case.n_row is not None:
        keep[case.n_row] = False
    return keep


@dataclass
class Report:
    needle_bad: set  # (sequence, row position, kv head) of the needle rows that miss their code
    needle_dev: float  # largest |out - code| over the needle rows that hit it
    named: dict  # bad needle -> the (position, kv head, sequence) its output names instead
    rel_bad: set  # (sequence, row in the packed q, head) over tau
    ratio: float | None  # largest relative error / f
    f: float | None
    tau: float | None
    close_err: float  # max |out - ref64| (today's close(atol 2e-2, rtol 2e-2) is also asserted)
    close_ok: bool

    @property
    def ok(self):
        return not self.needle_bad and not self.rel_bad and self.close_ok

    def __str__(self):
        return (f"needle rows off their code {sorted(self.needle_bad)} (naming {self.named}), largest deviation of the "
                f"rest {self.needle_dev:.3g}; relative check: {len(self.rel_bad)} rows over tau {self.tau} "
                f"(err / f {self.ratio}, f {self.f}) {sorted(self.rel_bad)[:8]}; max abs err {self.close_err:.3g}")


def check(case, out, tau_factor=TAU_FACTOR):
    """Needle / anti-needle rows against their codes, all other rows against the fp64 reference."""
    assert 0 < tau_factor <= 8
    out = out.reshape(case.q.shape)
    ref, _ = reference(case)
    G = case.Hq // case.Hkv
    bad, named, dev = set(), {}, 0.0
    if case.n_row is not None:
        d = (out[case.n_row].float() - case.n_exp.to(out.device)).abs().amax(-1)  # [R, Hq]
        miss = ~(d <= NEEDLE_TOL)  # NaN counts as a miss
        dev = float(d[~miss].max()) if (~miss).any() else 0.0
        for r, h in miss.nonzero().tolist():
            key = (int(case.n_seq[r]), int(case.n_pos[r]), h // G)
            bad.add(key)
            named.setdefault(key, decode_code(out[case.n_row[r], h]))
    f = emulation_floor(case)
    rel_bad, ratio, tau = set(), None, None
    if f is not None:
        tau = min(tau_factor * f, TAU_CAP)
        rel = rel_err(out, ref)
        rel = torch.where(plain_rows(case)[:, None], rel, torch.zeros_like(rel))
        ratio = float(rel.nan_to_num(float("inf")).max()) / f
        over = (~(rel <= tau)).nonzero().cpu()
        cu = torch.tensor(case.qlens).cumsum(0)
        seq = torch.bucketize(over[:, 0], cu, right=True)
        start = torch.cat([cu.new_zeros(1), cu])[seq]
        rel_bad = set(zip(seq.tolist(), (over[:, 0] - start).tolist(), over[:, 1].tolist()))
    o, rf = out.float(), ref.float()
    return Report(bad, dev, named, rel_bad, ratio, f, tau, float((o - rf).abs().nan_to_num(float("inf")).max()),
                  bool(torch.allclose(o, rf, atol=2e-2, rtol=2e-2)))


def needle_keys(case):
    """{(sequence, row position, kv head): needle key position} of a case."""
    if case.n_row is None:
        return {}
    return {(int(case.n_seq[r]), int(case.n_pos[r]), hk): int(case.n_key[r, hk])
            for r in range(case.n_row.numel()) for hk in range(case.Hkv)}


def run(case, ops, **kw):
    """The case through ``ops`` (CPU tensors: the fp32 oracle; device tensors: the HIP kernels)."""
    if case.kind == "decode":
        kw.setdefault("part_size", case.part)
        return ops.paged_decode(case.q, case.k, case.v, case.bt, case.ctx, scale=case.scale, **kw)
    if case.kind == "paged":
        return ops.flash_attention_paged(case.q, case.k, case.v, case.bt, case.cu_q, case.ctx, max(case.qlens),
                                         causal=case.causal, scale=case.scale, **kw)
    return ops.flash_attention_packed(case.q, case.k, case.v, case.cu_q, case.cu_k, max(case.qlens), causal=case.causal,
                                      scale=case.scale, **kw)
