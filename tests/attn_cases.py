"""Shared case builders and fp64 oracles for the paged-attention edge tests
and the decode-step chain tests (plain module, no tests of its own).

Conventions
  * every input is a bf16-valued tensor; the oracles upcast to fp64 and
    their output is the truth ``T``
  * ``W`` is the project's CPU path (``ops.*`` on CPU tensors: fp32 math,
    bf16 storage) on the same inputs, ``K`` the HIP kernel
  * ``err(X) = max|X - T| / max|T|``; a kernel passes when
    ``err(K) <= MARGIN * err(W)`` (see ``budget_check``)

Needle inputs: each KV head has a direction ``n`` (entries +-1), queries are
``n + randn``, selected cache positions hold the key ``c * n`` (c = 3 for
positions a row may see, c = 4 for positions no row may see), everything
else is ``randn``.  With D = 128 a visible needle takes essentially all of
the softmax weight, so a mask / length / window / page error of ONE position
at a needle moves the output by O(1) instead of O(0.01).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

D = 128
BF = torch.bfloat16
F64 = torch.float64

# err(K) <= MARGIN * err(W): the kernels may round to bf16 up to three times
# where the CPU path rounds once (unscaled QKV stored then scaled+rotated; P
# rounded before PV in prefill; output rounding), plus one unit for fp32
# accumulation order and __expf.
MARGIN = 4.0

# af_attn_decode (csrc/attn_decode.hip) picks the WIDE loop when
# B * Hk * nsplit >= 1024 workgroups, the narrow one below.
WIDE_MIN_WG = 1024

C_IN = 3.0     # needle a row is allowed to see
C_OUT = 4.0    # needle that must be ignored (stale slot, outside window, page 0)
V_LARGE = 1.0e4  # scale of the values parked in null page 0


def decode_arm(B: int, Hk: int, nsplit: int) -> str:
    return "WIDE" if B * Hk * nsplit >= WIDE_MIN_WG else "narrow"


def prefill_rows(G: int) -> int:
    """q rows per workgroup of attn_prefill_kernel<G> (ROWS)."""
    return 16 * max(1, 4 // G)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def randn_bf16(g: torch.Generator, *shape, scale: float = 1.0) -> torch.Tensor:
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def err(X: torch.Tensor, T: torch.Tensor) -> float:
    X = X.detach().cpu().to(F64)
    T = T.detach().cpu().to(F64)
    den = T.abs().max().item()
    d = (X - T).abs().max().item()
    if den == 0.0:
        return d
    return d / den


def budget_check(name: str, K, W, T, margin: float = MARGIN) -> float:
    """Assert err(K) <= margin * err(W); print both; return the ratio."""
    eK, eW = err(K, T), err(W, T)
    if eW > 0:
        ratio = eK / eW
    else:
        ratio = 0.0 if eK == 0 else float("inf")
    print(f"[budget] {name}: err(K)={eK:.3e} err(W)={eW:.3e} "
          f"ratio={ratio:.2f}")
    assert eK <= margin * eW, (
        f"{name}: err(K)={eK:.3e} > {margin} * err(W)={eW:.3e} "
        f"(ratio {ratio:.2f})")
    return ratio


def exceeds_budget(M, W, T, margin: float = MARGIN) -> bool:
    """True when a (mutated) result fails the pass criterion."""
    eM = err(M, T)
    return not (eM <= margin * err(W, T))


# ------------------------------------------------------------------ oracles
def rstd64(ss: torch.Tensor, k_dim: int, eps: float) -> torch.Tensor:
    """rsqrt(sum(ss)/K + eps) over the 8 column-block partials, fp64."""
    return torch.rsqrt(ss.to(F64).reshape(-1, 8).sum(-1) / k_dim + eps)


def swiglu64(gate_up: torch.Tensor, rstd: torch.Tensor | None = None):
    x = gate_up.to(F64)
    if rstd is not None:
        x = x * rstd[:, None]
    I = x.shape[-1] // 2
    g, u = x[:, :I], x[:, I:]
    return g / (1.0 + torch.exp(-g)) * u


def rope64(x: torch.Tensor, positions: torch.Tensor, table: torch.Tensor):
    """Rotate-half RoPE.  x [T, H, D] fp64, table [P, D] = [cos | sin]."""
    half = x.shape[-1] // 2
    tab = table.to(F64)[positions.long()]
    cos, sin = tab[:, None, :half], tab[:, None, half:]
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def rope_cache64(q, k, v, positions, table, kc64, vc64, slots,
                 rstd: torch.Tensor | None = None):
    """fp64 rope + paged append.  q [T,Hq*D], k/v [T,Hk*D]; caches fp64
    [npages,Hk,page,D] are updated in place (slot < 0: no write).
    Returns rotated (q, k) and the (scaled) v."""
    _, Hk, page, Dh = kc64.shape
    q3 = q.to(F64).unflatten(-1, (-1, Dh))
    k3 = k.to(F64).unflatten(-1, (Hk, Dh))
    v3 = v.to(F64).unflatten(-1, (Hk, Dh))
    if rstd is not None:
        r = rstd[:, None, None]
        q3, k3, v3 = q3 * r, k3 * r, v3 * r
    q3 = rope64(q3, positions, table)
    k3 = rope64(k3, positions, table)
    for t in range(q3.shape[0]):
        s = int(slots[t])
        if s < 0:
            continue
        p, o = divmod(s, page)
        kc64[p, :, o] = k3[t]
        vc64[p, :, o] = v3[t]
    return q3.flatten(1), k3.flatten(1), v3.flatten(1)


def _gather(c64, btrow, pos, page):
    """cache rows for absolute positions pos (LongTensor) -> [n, Hk, D]."""
    pg = btrow.long()[pos // page]
    return c64[pg, :, pos % page]


def _attend(qh, ks, vs, scale):
    """qh [Hq, D], ks/vs [n, Hk, D] -> [Hq, D]; empty n -> zeros."""
    Hq = qh.shape[0]
    if ks.shape[0] == 0:
        return torch.zeros(Hq, qh.shape[1], dtype=F64)
    G = Hq // ks.shape[1]
    k = ks.permute(1, 0, 2).repeat_interleave(G, dim=0)   # [Hq, n, D]
    v = vs.permute(1, 0, 2).repeat_interleave(G, dim=0)
    s = torch.einsum("hnd,hd->hn", k, qh) * scale
    return torch.einsum("hn,hnd->hd", s.softmax(-1), v)


# Mutations of the oracles: each models one boundary defect of a kernel.
DECODE_MUTANTS = ("win+1", "win-1", "drop_last", "admit_L",
                  "drop_split_first", "wrong_last_page", "page0")
PREFILL_MUTANTS = ("win+1", "win-1", "diag_dropped", "next_admitted",
                   "tile_last_row_short", "wrong_last_page", "page0")


def paged_decode64(q, kc64, vc64, bt, lens, scale, window=0, nsplit=1,
                   mut: str | None = None):
    """fp64 paged decode attention.  q [B, Hq*D] -> [B, Hq*D].
    Same semantics as ops.reference.attn_decode (window > 0: last `window`
    tokens only).  `mut` selects one deliberate defect (DECODE_MUTANTS)."""
    _, Hk, page, Dh = kc64.shape
    B = q.shape[0]
    q3 = q.to(F64).unflatten(-1, (-1, Dh))
    out = torch.zeros_like(q3)
    win = window
    if window > 0 and mut == "win+1":
        win = window + 1
    if window > 0 and mut == "win-1":
        win = window - 1
    for b in range(B):
        L = int(lens[b])
        s0 = L - win if (win > 0 and L > win) else 0
        pos = list(range(s0, L))
        if mut == "drop_last":
            pos = pos[:-1]
        elif mut == "admit_L":
            pos.append(L)
        elif mut == "drop_split_first" and nsplit > 1:
            chunk = (L - s0 + nsplit - 1) // nsplit
            if s0 + chunk < L:
                pos.remove(s0 + chunk)
        btrow = bt[b].clone()
        npg = (L + page - 1) // page
        if mut == "wrong_last_page" and L % page != 0:
            btrow[npg - 1] = btrow[npg - 2] if npg >= 2 else 0
        if mut == "page0":       # the block-table entry after the last used page
            pos.extend(range(npg * page, (npg + 1) * page))
        p = torch.tensor(pos, dtype=torch.long)
        out[b] = _attend(q3[b], _gather(kc64, btrow, p, page),
                         _gather(vc64, btrow, p, page), scale)
    return out.flatten(1)


def paged_prefill64(q, kc64, vc64, bt, q_start, cu, scale, window=0,
                    mut: str | None = None):
    """fp64 paged causal / windowed prefill.  Same semantics as
    ops.reference.attn_prefill_paged: key kpos is masked for the row at
    absolute position qpos when kpos > qpos or (window > 0 and
    kpos <= qpos - window)."""
    _, Hk, page, Dh = kc64.shape
    q3 = q.to(F64).unflatten(-1, (-1, Dh))
    Hq = q3.shape[1]
    G = Hq // Hk
    out = torch.zeros_like(q3)
    win = window
    if window > 0 and mut == "win+1":
        win = window + 1
    if window > 0 and mut == "win-1":
        win = window - 1
    cs = [int(x) for x in cu]
    for i in range(len(cs) - 1):
        a0, a1 = cs[i], cs[i + 1]
        n = a1 - a0
        hist = int(q_start[i])
        total = hist + n
        npg = (total + page - 1) // page
        btrow = bt[i].clone()
        if mut == "wrong_last_page" and total % page != 0:
            btrow[npg - 1] = btrow[npg - 2] if npg >= 2 else 0
        # one position past the end is gathered too: visible only to mutants
        kpos = torch.arange(total + 1)
        extra = torch.zeros(0, dtype=torch.long)
        if mut == "page0":
            extra = torch.arange(npg * page, (npg + 1) * page)
        allpos = torch.cat([kpos, extra])
        ks = _gather(kc64, btrow, allpos, page)       # [n_k, Hk, D]
        vs = _gather(vc64, btrow, allpos, page)
        kf = ks.permute(1, 0, 2).repeat_interleave(G, dim=0)
        vf = vs.permute(1, 0, 2).repeat_interleave(G, dim=0)
        qf = q3[a0:a1].permute(1, 0, 2)               # [Hq, n, D]
        att = torch.einsum("hqd,hkd->hqk", qf, kf) * scale
        qpos = torch.arange(hist, total)[:, None]
        kp = kpos[None, :]
        if mut == "diag_dropped":
            bad = kp > qpos - 1
        elif mut == "next_admitted":
            bad = kp > qpos + 1
        else:
            bad = kp > qpos
        if mut == "tile_last_row_short":
            r = torch.arange(n)[:, None]
            bad = bad | ((r % 16 == 15) & (kp == qpos))
        if win > 0:
            bad = bad | (kp <= qpos - win)
        bad = torch.cat([bad, torch.zeros(n, extra.numel(), dtype=torch.bool)],
                        dim=1)
        att = att.masked_fill(bad[None], float("-inf"))
        dead = bad.all(dim=1)                          # rows that see nothing
        att[:, dead] = 0.0
        o = torch.einsum("hqk,hkd->hqd", att.softmax(-1), vf)
        o[:, dead] = 0.0
        out[a0:a1] = o.permute(1, 0, 2)
    return out.flatten(1)


# ------------------------------------------------------------ decode cases
def _pages_for(lens_tokens, page, g):
    """Permuted block table with one spare (zero) column; page 0 is null."""
    npg = [(t + page - 1) // page for t in lens_tokens]
    total = 1 + sum(npg)
    perm = torch.randperm(total - 1, generator=g) + 1
    bt = torch.zeros(len(npg), max(npg) + 1, dtype=torch.int32)
    at = 0
    for b, n in enumerate(npg):
        bt[b, :n] = perm[at:at + n].to(torch.int32)
        at += n
    return bt, total


def _put_key(kc, bt, b, pos, page, n_dir, c):
    pg = int(bt[b, pos // page])
    kc[pg, :, pos % page] = (c * n_dir).to(BF)


def _fill_null_page(kc, vc, n_dir, g):
    kc[0] = (C_OUT * n_dir)[:, None, :].to(BF)
    vc[0] = randn_bf16(g, *vc[0].shape, scale=V_LARGE)


@dataclass
class DecodeCase:
    name: str
    Hq: int
    Hk: int
    page: int
    nsplit: int
    window: int
    lens: list
    qkv: torch.Tensor          # [B, (Hq+2Hk)*D] bf16; q is a strided view
    kc: torch.Tensor
    vc: torch.Tensor
    bt: torch.Tensor
    real: torch.Tensor         # bool [B]: rows that are compared
    strided: bool = True
    _t: dict = field(default_factory=dict)

    @property
    def B(self):
        return len(self.lens)

    @property
    def arm(self):
        return decode_arm(self.B, self.Hk, self.nsplit)

    @property
    def scale(self):
        return 1.0 / math.sqrt(D)

    def q_of(self, qkv):
        q = qkv[:, :self.Hq * D]
        return q if self.strided else q.contiguous()

    @property
    def q(self):
        return self.q_of(self.qkv)

    @property
    def lens_t(self):
        return torch.tensor(self.lens, dtype=torch.int32)

    def oracle(self, mut=None, lens=None):
        key = (mut, None if lens is None else tuple(lens))
        if key not in self._t:
            if "kc64" not in self._t:
                self._t["kc64"] = self.kc.to(F64)
                self._t["vc64"] = self.vc.to(F64)
            self._t[key] = paged_decode64(
                self.q, self._t["kc64"], self._t["vc64"], self.bt,
                self.lens if lens is None else lens, self.scale,
                self.window, self.nsplit, mut)
        return self._t[key]

    def cpu_path(self, lens=None):
        from agentfield_amd import ops
        key = ("W", None if lens is None else tuple(lens))
        if key not in self._t:
            lt = self.lens_t if lens is None else torch.tensor(
                lens, dtype=torch.int32)
            self._t[key] = ops.attn_decode(self.q, self.kc, self.vc, self.bt,
                                           lt, window=self.window)
        return self._t[key]


def make_decode_case(name, Hq, Hk, lens, page=16, nsplit=1, window=0,
                     seed=0, needles=True, strided=True, padded=()):
    """lens: tokens per row.  padded: row indices built as the engine builds
    padded graph lanes (len 1, block table all zero -> null page 0)."""
    g = gen(seed)
    B = len(lens)
    G = Hq // Hk
    lens = list(lens)
    for b in padded:
        lens[b] = 1
    # one spare slot per row so position L always has a page to be stale in
    bt, npages = _pages_for([l + 1 for l in lens], page, g)
    kc = randn_bf16(g, npages, Hk, page, D)
    vc = randn_bf16(g, npages, Hk, page, D)
    n_dir = torch.randint(0, 2, (Hk, D), generator=g).to(torch.float32) * 2 - 1
    qkv = randn_bf16(g, B, (Hq + 2 * Hk) * D)
    real = torch.ones(B, dtype=torch.bool)
    if needles:
        qn = n_dir.repeat_interleave(G, dim=0).flatten()[None, :]
        qkv[:, :Hq * D] = (qn + torch.randn(B, Hq * D, generator=g)).to(BF)
        _fill_null_page(kc, vc, n_dir, g)
    for b in padded:
        bt[b] = 0
        real[b] = False
    if needles:
        for b, L in enumerate(lens):
            if not real[b]:
                continue
            s0 = L - window if (window > 0 and L > window) else 0
            cand = [s0, L - 1]
            chunk = (L - s0 + nsplit - 1) // nsplit
            for s in range(nsplit):
                t0 = s0 + s * chunk
                t1 = min(L, t0 + chunk)
                if t0 < t1:
                    cand += [t0, t1 - 1]
            for p in range(s0, L):
                if p % page == 0 or p % page == page - 1:
                    cand.append(p)
            cand = list(dict.fromkeys(cand))
            picks = {cand[b % len(cand)], cand[(7 * b + 3) % len(cand)]}
            if s0 > 0:          # window active: first visible token always
                picks.add(s0)
            for p in picks:
                _put_key(kc, bt, b, p, page, n_dir, C_IN)
            # stale slots after the length, to the end of that page
            for p in range(L, (L // page + 1) * page):
                _put_key(kc, bt, b, p, page, n_dir, C_OUT)
            if s0 > 0:          # just outside the window
                _put_key(kc, bt, b, s0 - 1, page, n_dir, C_OUT)
    return DecodeCase(name, Hq, Hk, page, nsplit, window, lens, qkv, kc, vc,
                      bt, real, strided)


LENS_SWEEP = list(range(1, 65)) + [65, 127, 128, 129, 200]
LENS_TAILS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 200]


def _cycle(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


def _win_lens(win, n):
    # L < win, L = win, L = win+1, L = win+2, L >> win
    return _cycle([win - 3, win, win + 1, win + 2, 4 * win + 5, 200], n)


# name -> (kwargs, expected arm).  Smallest shapes that reach each arm.
DECODE_SPECS = {
    # WIDE arm, every G; the full length sweep (all tails of the 4-, 16- and
    # 32-token strides)
    "wide_g1_sweep": (dict(Hq=8, Hk=8, nsplit=1, seed=101,
                           lens=LENS_SWEEP + _cycle([66, 97, 150, 31], 59)),
                      "WIDE"),                         # 128*8*1 = 1024
    "wide_g2_sweep": (dict(Hq=4, Hk=2, nsplit=8, seed=102, lens=LENS_SWEEP),
                      "WIDE"),                         # 69*2*8 = 1104
    "wide_g4_sweep": (dict(Hq=8, Hk=2, nsplit=8, seed=103, lens=LENS_SWEEP),
                      "WIDE"),
    "wide_g8_sweep": (dict(Hq=8, Hk=1, nsplit=16, seed=104, lens=LENS_SWEEP),
                      "WIDE"),                         # 69*1*16 = 1104
    "wide_g2_b64": (dict(Hq=4, Hk=2, nsplit=8, seed=105,
                         lens=_cycle(LENS_TAILS, 64)), "WIDE"),
    "wide_g4_hk8": (dict(Hq=32, Hk=8, nsplit=8, seed=106, lens=LENS_TAILS),
                    "WIDE"),                           # 16*8*8 = 1024
    "wide_g8_hk8": (dict(Hq=64, Hk=8, nsplit=16, seed=107,
                         lens=[200, 3, 17, 33, 64, 65, 129, 1]), "WIDE"),
    "wide_g1_random": (dict(Hq=8, Hk=8, nsplit=1, seed=108, needles=False,
                            lens=_cycle(LENS_SWEEP, 128)), "WIDE"),
    "wide_g4_random": (dict(Hq=8, Hk=2, nsplit=8, seed=109, needles=False,
                            lens=LENS_SWEEP), "WIDE"),
    # one row short of the threshold: 127*8*1 = 1016 stays narrow
    "narrow_below_threshold": (dict(Hq=8, Hk=8, nsplit=1, seed=110,
                                    lens=_cycle(LENS_SWEEP, 127)), "narrow"),
    # the same lengths on the narrow arm (B=64, Hk=2, nsplit=1)
    "narrow_sweep_a": (dict(Hq=4, Hk=2, nsplit=1, seed=111,
                            lens=LENS_SWEEP[:64]), "narrow"),
    "narrow_sweep_b": (dict(Hq=8, Hk=2, nsplit=1, seed=112,
                            lens=_cycle(LENS_SWEEP[64:] + LENS_TAILS, 64)),
                       "narrow"),
    "narrow_g8": (dict(Hq=8, Hk=1, nsplit=4, seed=113, lens=LENS_TAILS),
                     "narrow"),
    "narrow_g1": (dict(Hq=2, Hk=2, nsplit=2, seed=114, lens=LENS_TAILS),
                  "narrow"),
    "narrow_random": (dict(Hq=8, Hk=2, nsplit=4, seed=115, needles=False,
                           lens=LENS_TAILS), "narrow"),
    # nsplit > L: mostly empty splits (first decode step after a short prompt)
    "wide_empty_splits": (dict(Hq=2, Hk=1, nsplit=16, seed=120,
                               lens=_cycle([1, 3, 15], 64)), "WIDE"),
    "wide_empty_splits_win": (dict(Hq=2, Hk=1, nsplit=16, window=8, seed=121,
                                   lens=_cycle([1, 3, 15], 64)), "WIDE"),
    "narrow_empty_splits": (dict(Hq=2, Hk=1, nsplit=16, seed=122,
                                 lens=_cycle([1, 3, 15], 9)), "narrow"),
    "narrow_empty_splits_win": (dict(Hq=2, Hk=1, nsplit=16, window=8,
                                     seed=123, lens=_cycle([1, 3, 15], 9)),
                                "narrow"),
    # page sizes 4 (engine tests) and 64 (engine default)
    "wide_page4": (dict(Hq=4, Hk=2, nsplit=8, page=4, seed=130,
                        lens=_cycle(LENS_TAILS, 64)), "WIDE"),
    "wide_page64": (dict(Hq=4, Hk=2, nsplit=8, page=64, seed=131,
                         lens=_cycle(LENS_TAILS, 64)), "WIDE"),
    "narrow_page4": (dict(Hq=8, Hk=2, nsplit=2, page=4, seed=132,
                          lens=LENS_TAILS), "narrow"),
    "narrow_page64": (dict(Hq=8, Hk=2, nsplit=2, page=64, seed=133,
                           lens=LENS_TAILS), "narrow"),
    # sliding window: L < win, = win, = win+1, >> win; nsplit > 1
    "wide_win16": (dict(Hq=4, Hk=2, nsplit=8, window=16, seed=140,
                        lens=_win_lens(16, 64)), "WIDE"),
    "wide_win33": (dict(Hq=8, Hk=1, nsplit=16, window=33, seed=141,
                        lens=_win_lens(33, 64)), "WIDE"),
    "narrow_win16": (dict(Hq=4, Hk=2, nsplit=4, window=16, seed=142,
                          lens=_win_lens(16, 12)), "narrow"),
    "narrow_win33": (dict(Hq=8, Hk=2, nsplit=2, window=33, page=4, seed=143,
                          lens=_win_lens(33, 12)), "narrow"),
    # padded lanes as the engine builds them (len 1, block table -> page 0)
    "wide_padded": (dict(Hq=4, Hk=2, nsplit=8, seed=150,
                         lens=_cycle(LENS_TAILS, 64),
                         padded=tuple(range(40, 64)) + (0, 7)), "WIDE"),
    "narrow_padded": (dict(Hq=4, Hk=2, nsplit=4, seed=151,
                           lens=_cycle(LENS_TAILS, 8), padded=(0, 5, 6, 7)),
                      "narrow"),
}

_DECODE_CACHE: dict = {}


def decode_case(name: str) -> DecodeCase:
    if name not in _DECODE_CACHE:
        kw, arm = DECODE_SPECS[name]
        c = make_decode_case(name, **kw)
        assert c.arm == arm, (name, c.arm, arm)
        _DECODE_CACHE[name] = c
    return _DECODE_CACHE[name]


# ----------------------------------------------------------- prefill cases
@dataclass
class PrefillCase:
    name: str
    Hq: int
    Hk: int
    page: int
    window: int
    hists: list
    lens: list                 # chunk rows per sequence
    qkv: torch.Tensor          # [T, (Hq+2Hk)*D]; q is a strided view
    kc: torch.Tensor
    vc: torch.Tensor
    bt: torch.Tensor
    _t: dict = field(default_factory=dict)

    @property
    def scale(self):
        return 1.0 / math.sqrt(D)

    def q_of(self, qkv):
        return qkv[:, :self.Hq * D]

    @property
    def q(self):
        return self.q_of(self.qkv)

    @property
    def q_start(self):
        return torch.tensor(self.hists, dtype=torch.int32)

    @property
    def cu(self):
        cu = [0]
        for n in self.lens:
            cu.append(cu[-1] + n)
        return torch.tensor(cu, dtype=torch.int32)

    def oracle(self, mut=None):
        if mut not in self._t:
            if "kc64" not in self._t:
                self._t["kc64"] = self.kc.to(F64)
                self._t["vc64"] = self.vc.to(F64)
            self._t[mut] = paged_prefill64(
                self.q, self._t["kc64"], self._t["vc64"], self.bt,
                self.hists, self.cu, self.scale, self.window, mut)
        return self._t[mut]

    def cpu_path(self):
        from agentfield_amd import ops
        if "W" not in self._t:
            self._t["W"] = ops.attn_prefill(
                self.q, self.kc, self.vc, self.bt, self.q_start, self.cu,
                self.lens, window=self.window)
        return self._t["W"]


def make_prefill_case(name, Hq, Hk, hists, lens, page=16, window=0, seed=0,
                      needles=True):
    g = gen(seed)
    G = Hq // Hk
    rows = prefill_rows(G)
    S = len(lens)
    totals = [h + n for h, n in zip(hists, lens)]
    bt, npages = _pages_for([t + 1 for t in totals], page, g)
    kc = randn_bf16(g, npages, Hk, page, D)
    vc = randn_bf16(g, npages, Hk, page, D)
    n_dir = torch.randint(0, 2, (Hk, D), generator=g).to(torch.float32) * 2 - 1
    T = sum(lens)
    qkv = randn_bf16(g, T, (Hq + 2 * Hk) * D)
    if needles:
        qn = n_dir.repeat_interleave(G, dim=0).flatten()[None, :]
        qkv[:, :Hq * D] = (qn + torch.randn(T, Hq * D, generator=g)).to(BF)
        _fill_null_page(kc, vc, n_dir, g)
        for s in range(S):
            h, n, tot = hists[s], lens[s], totals[s]
            # rows at the 16-row and ROWS tile edges (chunk-relative)
            edge = [r for r in dict.fromkeys(
                [0, 15, 16, rows - 1, rows, n - 1]) if 0 <= r < n]
            inside = [h + r for r in edge]                 # the diagonal
            inside += [p for p in (63, 64) if p < tot]     # KV tile edges
            # stale slots after the end, to the end of that page
            never = list(range(tot, (tot // page + 1) * page))
            if window > 0:
                for r in edge:
                    a = h + r
                    if a - window + 1 >= 0:
                        inside.append(a - window + 1)      # first visible
                    if a - window >= 0:
                        # just outside row r's window: the row before still
                        # sees it; below row 0's window no row does
                        (inside if r > 0 else never).append(a - window)
            never = set(never)
            for p in dict.fromkeys(inside):
                if p not in never:
                    _put_key(kc, bt, s, p, page, n_dir, C_IN)
            for p in never:
                _put_key(kc, bt, s, p, page, n_dir, C_OUT)
    return PrefillCase(name, Hq, Hk, page, window, list(hists), list(lens),
                       qkv, kc, vc, bt)


PREFILL_LENS = [1, 15, 16, 17, 63, 64, 65, 129]
CHUNK_HISTS = [0, 1, 63, 64, 65, 130]
CHUNK_LENS = [1, 2, 5, 17, 64]


def _chunk_grid(hists, lens):
    hs, ls = [], []
    for h in hists:
        for n in lens:
            hs.append(h)
            ls.append(n)
    return hs, ls


def _build_prefill_specs():
    specs = {}
    # full prompts crossing 16 rows, ROWS (64/32/16/16) and the 64-token
    # KV tile, at every G and the three page sizes in use
    for G in (1, 2, 4, 8):
        for page in (4, 16, 64):
            specs[f"full_g{G}_page{page}"] = dict(
                Hq=2 * G, Hk=2, hists=[0] * len(PREFILL_LENS),
                lens=PREFILL_LENS, page=page, seed=200 + 10 * G + page)
    specs["full_g4_random"] = dict(Hq=8, Hk=2, hists=[0] * 8,
                                   lens=PREFILL_LENS, seed=290, needles=False)
    # chunked prefill, several sequences per call (speculative verify uses
    # chunks of 1-5 rows)
    hs, ls = _chunk_grid(CHUNK_HISTS, CHUNK_LENS)
    for G, page in ((1, 64), (2, 4), (4, 16), (8, 16)):
        specs[f"chunk_g{G}_page{page}"] = dict(
            Hq=2 * G, Hk=2, hists=hs, lens=ls, page=page, seed=300 + G)
    specs["chunk_g2_random"] = dict(Hq=4, Hk=2, hists=hs, lens=ls, page=16,
                                    seed=390, needles=False)
    # chunked + sliding window with hist > win (kt_first > 0)
    for win in (16, 64, 65):
        whs, wls = _chunk_grid([win + 1, 130, 200], [1, 5, 17, 64])
        for G in (1, 2, 4, 8):
            specs[f"chunk_win{win}_g{G}"] = dict(
                Hq=G, Hk=1, hists=whs, lens=wls, window=win,
                page=(4 if G == 2 else 16), seed=400 + win + G)
    specs["chunk_win64_random"] = dict(
        Hq=8, Hk=2, hists=[65, 130, 200, 200], lens=[64, 17, 5, 70],
        window=64, seed=490, needles=False)
    # full prompt + window (history 0, band starts inside the chunk)
    specs["full_win16_g2"] = dict(Hq=4, Hk=2, hists=[0] * 4,
                                  lens=[15, 17, 65, 129], window=16, seed=495)
    return specs


PREFILL_SPECS = _build_prefill_specs()
_PREFILL_CACHE: dict = {}


def prefill_case(name: str) -> PrefillCase:
    if name not in _PREFILL_CACHE:
        _PREFILL_CACHE[name] = make_prefill_case(name, **PREFILL_SPECS[name])
    return _PREFILL_CACHE[name]


# ------------------------------------------------- decode-step chain helpers
def skinny_cpu(x, w, mode=0, residual=None, scale=None):
    """fp32-math / bf16-storage counterpart of ops.linear_skinny (which has
    no CPU path): one fp32 GEMM, epilogue in fp32, one rounding to bf16.
    mode 1/4 update `residual` in place like the kernel."""
    acc = x.float() @ w.float().t()
    if scale is not None:
        ss, eps = scale
        rstd = torch.rsqrt(ss.float().view(-1, 8).sum(-1) / x.shape[1] + eps)
        acc = acc * rstd[:, None]
    if mode == 2:
        I = acc.shape[1] // 2
        return (torch.nn.functional.silu(acc[:, :I]) * acc[:, I:]).to(x.dtype)
    if mode in (1, 4):
        out = (acc + residual.float()).to(x.dtype)
        residual.copy_(out)
        return out
    return acc.to(x.dtype)


def colblock_ss64(out_bf16: torch.Tensor) -> torch.Tensor:
    """[M, N] -> [M, 8] fp64 sum of squares per column block of N/8."""
    M, N = out_bf16.shape
    return out_bf16.to(F64).pow(2).view(M, 8, N // 8).sum(-1)


def llama_decode64(sd, cfg, ids, positions, kcs, vcs, bt, lens, slots, table):
    """fp64 Llama decode forward (dense, norms folded or not).  sd: state
    dict upcast to fp64; kcs/vcs: per-layer fp64 caches, updated in place.
    Returns logits [B, V]."""
    eps = cfg.rms_eps
    scale = 1.0 / math.sqrt(cfg.head_dim)
    qs, ks = cfg.q_size, cfg.kv_size

    def norm(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w

    x = sd["embed"][ids.long()]
    for i in range(cfg.num_layers):
        p = f"layers.{i}."
        qkv = norm(x, sd[p + "input_norm"]) @ sd[p + "attn.qkv"].t()
        q, _, _ = rope_cache64(qkv[:, :qs], qkv[:, qs:qs + ks],
                               qkv[:, qs + ks:], positions, table,
                               kcs[i], vcs[i], slots)
        o = paged_decode64(q, kcs[i], vcs[i], bt, lens, scale)
        x = x + o @ sd[p + "attn.o"].t()
        gu = norm(x, sd[p + "post_norm"]) @ sd[p + "mlp.gate_up"].t()
        x = x + swiglu64(gu) @ sd[p + "mlp.down"].t()
    return norm(x, sd["final_norm"]) @ sd["lm_head"].t()


STEP_CTX = [0, 1, 3, 15, 16, 17, 31, 63, 64, 65, 100]   # cached tokens / row
STEP_NSPLIT = 8     # B=128, Hk=1 -> 128*1*8 = 1024 workgroups: the WIDE arm


@dataclass
class StepCase:
    """One decode step of CONFIGS["tiny"] (random norm weights, folded) over
    a prefilled cache with mixed lengths."""
    cfg: object
    model: object              # CPU model, norms folded
    ids: torch.Tensor
    pos: torch.Tensor
    slots: torch.Tensor
    bt: torch.Tensor
    lens: torch.Tensor
    kcs: list
    vcs: list
    page: int
    _t: dict = field(default_factory=dict)

    def metadata(self, dev="cpu"):
        from agentfield_amd.models.llama import AttnMetadata
        return AttnMetadata(is_prefill=False, slots=self.slots.to(dev),
                            block_table=self.bt.to(dev),
                            seq_lens_t=self.lens.to(dev), nsplit=STEP_NSPLIT)

    def kv(self, dev="cpu"):
        from agentfield_amd.models.llama import KVCache
        kv = KVCache(self.cfg, self.kcs[0].shape[0], self.page, dev)
        for i in range(self.cfg.num_layers):
            kv.k[i].copy_(self.kcs[i])
            kv.v[i].copy_(self.vcs[i])
        return kv

    def oracle(self):
        if "T" not in self._t:
            sd = {k: v.to(F64) for k, v in self.model.state_dict().items()}
            self._t["T"] = llama_decode64(
                sd, self.cfg, self.ids, self.pos,
                [k.to(F64) for k in self.kcs], [v.to(F64) for v in self.vcs],
                self.bt, self.lens.tolist(), self.slots.tolist(),
                self.model.rope_tab)
        return self._t["T"]

    def cpu_path(self):
        if "W" not in self._t:
            with torch.no_grad():
                self._t["W"] = self.model(self.ids, self.pos, self.kv("cpu"),
                                          self.metadata("cpu"))
        return self._t["W"]


_STEP_CACHE: dict = {}


def step_case(B: int, seed: int = 7, page: int = 16) -> StepCase:
    if B in _STEP_CACHE:
        return _STEP_CACHE[B]
    from agentfield_amd.models import CONFIGS
    from agentfield_amd.models.llama import LlamaForCausalLM
    cfg = CONFIGS["tiny"]
    g = gen(seed + B)
    model = LlamaForCausalLM(cfg, device="cpu").init_random(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_((1 + 0.1 * torch.randn(p.shape, generator=g)).to(BF))
    model.fold_norm_weights()
    ctx = _cycle(STEP_CTX, B)
    lens = [c + 1 for c in ctx]
    bt, npages = _pages_for(lens, page, g)
    shape = (npages, cfg.num_kv_heads, page, cfg.head_dim)
    kcs = [randn_bf16(g, *shape, scale=0.3) for _ in range(cfg.num_layers)]
    vcs = [randn_bf16(g, *shape, scale=0.3) for _ in range(cfg.num_layers)]
    ids = torch.randint(0, cfg.vocab_size, (B,), generator=g).to(torch.int32)
    slots = torch.tensor([int(bt[b, c // page]) * page + c % page
                          for b, c in enumerate(ctx)], dtype=torch.int64)
    c = StepCase(cfg, model, ids, torch.tensor(ctx, dtype=torch.int32), slots,
                 bt, torch.tensor(lens, dtype=torch.int32), kcs, vcs, page)
    _STEP_CACHE[B] = c
    return c
