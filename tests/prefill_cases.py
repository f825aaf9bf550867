"""Case builders and fp64 oracles for the prefill-sized arms of the row
kernels: RMSNorm, RoPE + cache append, cache scatter, embedding, SwiGLU, add,
row gather, and one prefill step of the model (plain module, no tests of its
own).  Conventions are those of ``attn_cases``: ``T`` is the fp64 oracle on
bf16-valued inputs, ``W`` the project's CPU path, ``K`` the HIP kernel, and a
kernel passes when ``err(K) <= MARGIN * err(W)``.

Per-row error: every kernel here treats a row as an independent problem, so
the error is taken per row (``row_err``); with the global maximum a row whose
scalar is off by a few percent hides behind the largest row of the tensor.

Row inputs: row t is ``randn * 2^((t % 7) - 3)``, so a kernel that gives row t
another row's statistic (or another row's result) is off by a factor >= 2.

The launch rules of the kernels are restated as small pure functions
(``rmsnorm_arm`` ... ``gather_trips``); every case records the arm it claims
and ``test_prefill_cases_cpu.py`` checks the claim against those functions.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

from attn_cases import (BF, D, F64, MARGIN, _pages_for, err, gen,
                        paged_prefill64, randn_bf16, rope_cache64, rstd64,
                        swiglu64)

EPS = 1e-5
NTHR = 256
RMS_CAP = 16384      # rmsnorm_kernel grid cap (rows)
ROW_CAP = 2048       # rope_cache / reshape_and_cache / embedding grid cap
VEC_CAP_BLOCKS = 2048                # silu_mul / add grid cap (blocks)
VEC_CAP = VEC_CAP_BLOCKS * NTHR      # = 524288 vectors of 8 in one trip
ROPE_MAX_POS = 8192                  # Llama-3 max_position


def _cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ------------------------------------------------------------- launch rules
def rmsnorm_arm(T: int) -> str:
    # rmsnorm.hip, af_rmsnorm: `if (T <= 256 && H <= 16384)` -> wave kernel
    return "wave" if T <= 256 else "block"


def rmsnorm_iters(H: int):
    """(iterations of the unrolled loop that hold a column, threads in the
    last one) of rmsnorm_kernel."""
    # rmsnorm.hip, rmsnorm_kernel: `c = threadIdx.x + it * NTHR;
    # if (c >= per_row) break;` with per_row = H / 8, it < MAX_IT = 8
    per_row = H // 8
    its = _cdiv(per_row, NTHR)
    return its, per_row - (its - 1) * NTHR


def grid_rows(T: int, cap: int):
    """(blocks, trips of the `row += gridDim.x` loop) of a row-per-block
    kernel with a capped grid."""
    # rmsnorm.hip: `blocks = T < 16384 ? T : 16384`; rope.hip / cache.hip:
    # `blocks = T < 2048 ? T : 2048`, loop `for (t = blockIdx.x; t < T;
    # t += gridDim.x)`
    blocks = min(T, cap)
    return blocks, _cdiv(T, blocks)


def vec_blocks(nvec: int):
    """(blocks, trips of the grid-stride loop) over nvec 8-element vectors."""
    # activation.hip, af_silu_mul / af_add: `blocks = (nvec + 255) / 256;
    # if (blocks > 2048) blocks = 2048`, loop stride gridDim.x * blockDim.x
    blocks = min(_cdiv(nvec, NTHR), VEC_CAP_BLOCKS)
    return blocks, _cdiv(nvec, blocks * NTHR)


def silu_blocks(T: int, I: int):
    # activation.hip, silu_mul_kernel: `nvec = T * (I >> 3)`
    return vec_blocks(T * (I >> 3))


def inner_trips(work: int) -> int:
    # `for (i = threadIdx.x; i < work; i += blockDim.x)` with 256 threads
    return _cdiv(work, NTHR)


def rope_work(Hq: int, Hk: int, Dh: int = D) -> int:
    # rope.hip, rope_cache_kernel: `rope_work = (Hq + Hk) * qh4`,
    # qh4 = (D / 2) / 4
    return (Hq + Hk) * ((Dh >> 1) >> 2)


def vcopy_work(Hk: int, Dh: int = D) -> int:
    # rope.hip: `v_work = Hk * (D >> 3)`; cache.hip, reshape_and_cache_kernel:
    # `per_tok = Hk * D / 8`
    return Hk * (Dh >> 3)


def embed_work(H: int) -> int:
    # cache.hip, embedding_kernel: `per_row = H / 8`
    return H // 8


def gather_trips(H: int) -> int:
    # sampling.hip, gather_rows_kernel: `for (i = threadIdx.x * 8; i < H;
    # i += 256 * 8)`
    return _cdiv(H, NTHR * 8)


# ------------------------------------------------------------ the criterion
def _rows(X: torch.Tensor) -> torch.Tensor:
    X = X.detach().cpu().to(F64)
    return X.reshape(X.shape[0], -1) if X.dim() > 1 else X.reshape(1, -1)


def row_err(X: torch.Tensor, T: torch.Tensor) -> float:
    """max over rows of max_j|X - T| / max_j|T|; a row with max|T| = 0 counts
    its absolute error.  NaN anywhere in X gives NaN."""
    X, T = _rows(X), _rows(T)
    assert X.shape == T.shape, (X.shape, T.shape)
    d = (X - T).abs().amax(dim=1)
    den = T.abs().amax(dim=1)
    den = torch.where(den == 0, torch.ones_like(den), den)
    return (d / den).max().item()


def row_budget_check(name: str, K, W, T, margin: float = MARGIN) -> float:
    """budget_check with the per-row error."""
    eK, eW = row_err(K, T), row_err(W, T)
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
    """True when a (mutated) result fails row_budget_check."""
    return not (row_err(M, T) <= margin * row_err(W, T))


def kill_ratio(M, W, T) -> float:
    eM, eW = row_err(M, T), row_err(W, T)
    if eM != eM:
        return float("inf")
    return eM / eW if eW > 0 else (0.0 if eM == 0 else float("inf"))


# --------------------------------------------------------------- row inputs
def row_scale(T: int) -> torch.Tensor:
    return torch.exp2(((torch.arange(T) % 7) - 3).float())


def scaled_rows(g, T: int, H: int) -> torch.Tensor:
    """fp32 [T, H]: row t is randn * 2^((t % 7) - 3)."""
    return torch.randn(T, H, generator=g) * row_scale(T)[:, None]


def norm_weight(g, H: int) -> torch.Tensor:
    return (1 + 0.1 * torch.randn(H, generator=g)).to(BF)


def ss8(g, x: torch.Tensor) -> torch.Tensor:
    """[M,8] stats with eight distinct non-zero slots summing to ~sum(x^2)."""
    tot = x.float().pow(2).sum(-1, keepdim=True)
    w = torch.rand(x.shape[0], 8, generator=g) + 0.5
    return (tot * w / w.sum(-1, keepdim=True)).contiguous()


def nan_bf16(*shape) -> torch.Tensor:
    """bf16 tensor of quiet NaNs (bit pattern 0x7FC0)."""
    t = torch.full(shape, float("nan"), dtype=BF)
    assert int(t.view(torch.int16).flatten()[0]) == 0x7FC0
    return t


# ------------------------------------------------------------------ rmsnorm
RMS_MUTANTS = ("stride_alias", "beyond_cap_unwritten", "neighbour_stat",
               "wave_partial_dropped", "tail_iter_dropped",
               "tail_iter_sum_dropped", "eps_outside", "residual_not_added")


def rmsnorm64(x, w, eps=EPS, res=None, mut: str | None = None, wave: int = 0):
    """fp64 (residual-add) RMSNorm.  Returns (out, h) with h = x (+ res).
    `mut` selects one deliberate defect of the block kernel (RMS_MUTANTS)."""
    h = x.to(F64)
    if res is not None and mut != "residual_not_added":
        h = h + res.to(F64)
    T, H = h.shape
    sq = h.pow(2)
    vec = torch.arange(H) // 8                 # vector index c of a column
    its, _ = rmsnorm_iters(H)
    tail = vec >= (its - 1) * NTHR if H // 8 % NTHR else torch.zeros(
        H, dtype=torch.bool)
    if mut == "wave_partial_dropped":          # red[wave] never added
        sq = sq * (((vec % NTHR) >> 6) != wave)
    if mut in ("tail_iter_dropped", "tail_iter_sum_dropped"):
        sq = sq * ~tail
    mean = sq.sum(-1, keepdim=True) / H
    rstd = torch.rsqrt(mean + eps)
    if mut == "eps_outside":
        rstd = torch.rsqrt(mean) + eps
    if mut == "neighbour_stat":
        rstd = torch.roll(rstd, -1, 0)
    out = h * rstd * w.to(F64)
    if mut == "tail_iter_dropped":
        out[:, tail] = float("nan")
    if mut == "stride_alias" and T > RMS_CAP:
        out[RMS_CAP:] = out[:T - RMS_CAP].clone()
    if mut == "beyond_cap_unwritten":
        out[RMS_CAP:] = float("nan")
    return out, h


# name -> (T, H, claimed arm): arm, iterations holding a column, threads in
# the last iteration, trips of the row loop
RMS_SPECS = {
    "wave_last_T": (256, 264, ("wave", 1, 33, 1)),
    "block_thread0_only": (257, 8, ("block", 1, 1, 1)),
    "block_one_full_iter": (257, 2048, ("block", 1, 256, 1)),
    "block_tail_one_thread": (300, 2056, ("block", 2, 1, 1)),
    "block_eight_full_iters": (257, 16384, ("block", 8, 256, 1)),
    "block_step_shape": (2100, 256, ("block", 1, 32, 1)),
    "block_row_stride": (16400, 8, ("block", 1, 1, 2)),
    "block_row_stride_3trips": (33000, 8, ("block", 1, 1, 3)),
}


@dataclass
class RmsCase:
    name: str
    T: int
    H: int
    x: torch.Tensor
    w: torch.Tensor
    res: torch.Tensor | None
    tiny_row: int
    _t: dict = field(default_factory=dict)

    def oracle(self, mut=None, wave=0):
        """(out64, h64)."""
        key = (mut, wave)
        if key not in self._t:
            self._t[key] = rmsnorm64(self.x, self.w, EPS, self.res, mut, wave)
        return self._t[key]

    def cpu_path(self):
        """(out, new_residual or None); the inputs stay unchanged."""
        from agentfield_amd import ops
        if "W" not in self._t:
            if self.res is None:
                self._t["W"] = (ops.rmsnorm(self.x, self.w, EPS), None)
            else:
                self._t["W"] = ops.rmsnorm(self.x, self.w, EPS,
                                           residual=self.res.clone())
        return self._t["W"]


_RMS_CACHE: dict = {}


def rms_case(name: str, residual: bool) -> RmsCase:
    key = (name, residual)
    if key not in _RMS_CACHE:
        T, H, _ = RMS_SPECS[name]
        g = gen(6000 + 2 * list(RMS_SPECS).index(name) + int(residual))
        tiny = T - 2          # beyond the grid cap in the row-stride cases
        x = scaled_rows(g, T, H)
        r = scaled_rows(g, T, H) if residual else None
        # one row of magnitude 1e-3: mean(h^2) < eps, so where eps is added
        # matters
        x[tiny] = torch.randn(H, generator=g) * 1e-3
        if residual:
            r[tiny] = torch.randn(H, generator=g) * 1e-3
        if H // 8 % NTHR and H > NTHR * 8:
            # columns of the partial last iteration carry half of the sum of
            # squares: dropping them from the statistic alone is visible
            n = H - (H // 8 // NTHR) * NTHR * 8
            x[:, -n:] *= math.sqrt((H - n) / n)
            if residual:
                r[:, -n:] *= math.sqrt((H - n) / n)
        _RMS_CACHE[key] = RmsCase(name, T, H, x.to(BF), norm_weight(g, H),
                                  r.to(BF) if residual else None, tiny)
    return _RMS_CACHE[key]


# ------------------------------------------------- rope + cache / cache only
_ROPE_TAB: dict = {}


def rope_tab():
    from agentfield_amd import ops
    if "t" not in _ROPE_TAB:
        _ROPE_TAB["t"] = ops.rope_table(ROPE_MAX_POS, D)
    return _ROPE_TAB["t"]


ROW_MUTANTS = ("stride_alias", "beyond_cap_unwritten",
               "inner_loop_single_trip")

# name -> (T, Hq, Hk, claimed arm): trips of the row loop, of the rotation
# loop and of the v-copy loop
ROPE_SPECS = {
    "row_stride": (2100, 4, 2, (2, 1, 1)),
    "rot_loop_640": (5, 32, 8, (1, 3, 1)),
    "rot_loop_1024_vcopy_512": (5, 32, 32, (1, 4, 2)),
}
# name -> (T, Hk, claimed arm): trips of the row loop and of the copy loop
CACHE_SPECS = {
    "row_stride": (2100, 2, (2, 1)),
    "copy_loop_512": (5, 32, (1, 2)),
}


def _slots_for(g, T, page):
    """Permuted slots, every third one -1 (no cache write)."""
    npages = _cdiv(T, page) + 3
    slots = torch.randperm(npages * page, generator=g)[:T].to(torch.int64)
    skip = torch.arange(T) % 3 == 1
    slots[skip] = -1
    return npages, slots, skip


def slot_rows(c: torch.Tensor, slots: torch.Tensor) -> torch.Tensor:
    """cache [npages,Hk,page,D] -> the rows at `slots` as [n, Hk*D]."""
    page = c.shape[2]
    return c[slots // page, :, slots % page].flatten(1)


def rest_of(c: torch.Tensor, slots: torch.Tensor) -> torch.Tensor:
    """Every cache entry outside `slots`, flattened."""
    npages, _, page, _ = c.shape
    hit = torch.zeros(npages * page, dtype=torch.bool)
    hit[slots] = True
    return c[~hit.view(npages, 1, page, 1).expand_as(c)]


@dataclass
class RopeCase:
    """rope_cache on strided q/k/v views of a fused QKV buffer; with Hq = 0
    and `rope` False the same record describes a reshape_and_cache case
    (k/v contiguous [T,Hk,D], pure copy)."""
    name: str
    T: int
    Hq: int
    Hk: int
    scaled: bool
    page: int
    qkv: torch.Tensor          # [T, (Hq+2Hk)*D]
    pos: torch.Tensor
    slots: torch.Tensor
    skip: torch.Tensor
    kc0: torch.Tensor
    vc0: torch.Tensor
    ss: torch.Tensor | None
    kdim: int
    rope: bool = True
    _t: dict = field(default_factory=dict)

    @property
    def sl(self):
        a, b = self.Hq * D, (self.Hq + self.Hk) * D
        return slice(0, a), slice(a, b), slice(b, None)

    @property
    def written(self):
        return self.slots[~self.skip]

    def scale(self, ss):
        return (ss, self.kdim, EPS) if self.scaled else None

    def oracle(self):
        """dict q, k [T, *] and the full caches kc, vc, all fp64, plus v
        (the scaled v rows)."""
        if "T" not in self._t:
            kc, vc = self.kc0.to(F64), self.vc0.to(F64)
            sq, sk, sv = self.sl
            if self.rope:
                q, k, v = rope_cache64(
                    self.qkv[:, sq], self.qkv[:, sk], self.qkv[:, sv],
                    self.pos, rope_tab(), kc, vc, self.slots,
                    rstd64(self.ss, self.kdim, EPS) if self.scaled else None)
            else:
                q = self.qkv[:, sq].to(F64)
                k, v = self.qkv[:, sk].to(F64), self.qkv[:, sv].to(F64)
                for t in range(self.T):
                    _put(kc, vc, int(self.slots[t]), k[t], v[t])
            self._t["T"] = dict(q=q, k=k, v=v, kc=kc, vc=vc)
        return self._t["T"]

    def cpu_path(self):
        from agentfield_amd import ops
        if "W" not in self._t:
            qkv, kc, vc = self.qkv.clone(), self.kc0.clone(), self.vc0.clone()
            q, k, v = (qkv[:, s] for s in self.sl)
            if self.rope:
                ops.rope_cache(q, k, v, self.pos, rope_tab(), kc, vc,
                               self.slots, scale=self.scale(self.ss))
            else:
                ops.reshape_and_cache(
                    k.unflatten(-1, (self.Hk, D)).contiguous(),
                    v.unflatten(-1, (self.Hk, D)).contiguous(), kc, vc,
                    self.slots)
            self._t["W"] = dict(q=q, k=k, v=v, kc=kc, vc=vc)
        return self._t["W"]

    def mutant(self, mut: str):
        """The oracle's outputs with one defect of the launch structure."""
        T0 = self.oracle()
        R = {n: t.clone() for n, t in T0.items()}
        sq, sk, sv = self.sl
        q0, k0 = self.qkv[:, sq].to(F64), self.qkv[:, sk].to(F64)
        kc0, vc0 = self.kc0.to(F64), self.vc0.to(F64)
        page = self.page

        def restore(t, heads=slice(None)):
            s = int(self.slots[t])
            if s >= 0:
                p, o = divmod(s, page)
                R["kc"][p, heads, o] = kc0[p, heads, o]
                R["vc"][p, heads, o] = vc0[p, heads, o]

        if mut == "stride_alias":           # row t takes row t - cap's result
            for t in range(ROW_CAP, self.T):
                R["q"][t], R["k"][t] = T0["q"][t - ROW_CAP], T0["k"][t - ROW_CAP]
                _put(R["kc"], R["vc"], int(self.slots[t]),
                     T0["k"][t - ROW_CAP], T0["v"][t - ROW_CAP])
        elif mut == "beyond_cap_unwritten":
            for t in range(ROW_CAP, self.T):
                R["q"][t], R["k"][t] = q0[t], k0[t]
                restore(t)
        elif mut == "inner_loop_single_trip":
            # 256 rotation items of 4 pairs = the first 16 heads of [q | k];
            # 256 copy items of 8 elements = the first 16 kv heads
            done = NTHR * 8 // D
            if self.rope:
                R["q"][:, done * D:] = q0[:, done * D:]
                kdone = max(0, done - self.Hq)
                R["k"][:, kdone * D:] = k0[:, kdone * D:]
                for t in range(self.T):
                    s = int(self.slots[t])
                    if s >= 0:
                        p, o = divmod(s, page)
                        R["kc"][p, kdone:, o] = kc0[p, kdone:, o]
                        R["vc"][p, done:, o] = vc0[p, done:, o]
            else:
                for t in range(self.T):
                    restore(t, slice(done, None))
        else:
            raise ValueError(mut)
        return R

    def views(self, R):
        """Outputs as row tensors: in-place q/k rows, the written cache rows,
        and every cache entry that must keep its bits."""
        w = self.written
        out = dict(kc_rows=slot_rows(R["kc"], w), vc_rows=slot_rows(R["vc"], w),
                   kc_rest=rest_of(R["kc"], w), vc_rest=rest_of(R["vc"], w))
        if self.rope:
            out.update(q=R["q"], k=R["k"])
        return out

    def killed(self, R) -> float:
        """0 when result R passes every check of the GPU test, else the
        largest err(R)/err(W) (inf where bits had to match)."""
        Wv, Tv, Rv = (self.views(x) for x in (self.cpu_path(), self.oracle(),
                                               R))
        worst = 0.0
        for n in ("kc_rest", "vc_rest"):
            if not torch.equal(Rv[n], Tv[n]):
                worst = float("inf")
        for n in Rv:
            if not n.endswith("_rest") and exceeds_budget(Rv[n], Wv[n], Tv[n]):
                worst = max(worst, kill_ratio(Rv[n], Wv[n], Tv[n]))
        return worst


def _put(kc, vc, s, krow, vrow):
    if s < 0:
        return
    p, o = divmod(s, kc.shape[2])
    kc[p, :, o] = krow.view(kc.shape[1], -1)
    vc[p, :, o] = vrow.view(vc.shape[1], -1)


_ROPE_CACHE: dict = {}


def rope_case(name: str, scaled: bool) -> RopeCase:
    key = (name, scaled)
    if key not in _ROPE_CACHE:
        T, Hq, Hk, _ = ROPE_SPECS[name]
        g = gen(7000 + 2 * list(ROPE_SPECS).index(name) + int(scaled))
        page, kdim = 16, 256
        qkv = scaled_rows(g, T, (Hq + 2 * Hk) * D).to(BF)
        npages, slots, skip = _slots_for(g, T, page)
        pos = torch.randint(0, ROPE_MAX_POS, (T,), generator=g).to(torch.int32)
        pos[0], pos[T - 1] = ROPE_MAX_POS - 1, 0
        if T > ROW_CAP:
            pos[ROW_CAP + 1] = ROPE_MAX_POS - 1
        kc0 = randn_bf16(g, npages, Hk, page, D)
        vc0 = randn_bf16(g, npages, Hk, page, D)
        ss = ss8(g, qkv[:, :kdim]) if scaled else None
        _ROPE_CACHE[key] = RopeCase(name, T, Hq, Hk, scaled, page, qkv, pos,
                                    slots, skip, kc0, vc0, ss, kdim)
    return _ROPE_CACHE[key]


def cache_case(name: str) -> RopeCase:
    key = ("cache", name)
    if key not in _ROPE_CACHE:
        T, Hk, _ = CACHE_SPECS[name]
        g = gen(7500 + list(CACHE_SPECS).index(name))
        page = 16
        kv = scaled_rows(g, T, 2 * Hk * D).to(BF)
        npages, slots, skip = _slots_for(g, T, page)
        kc0 = randn_bf16(g, npages, Hk, page, D)
        vc0 = randn_bf16(g, npages, Hk, page, D)
        _ROPE_CACHE[key] = RopeCase(
            name, T, 0, Hk, False, page, kv, torch.zeros(T, dtype=torch.int32),
            slots, skip, kc0, vc0, None, 0, rope=False)
    return _ROPE_CACHE[key]


# ---------------------------------------------------------------- embedding
# name -> (T, H, claimed arm): trips of the row loop and of the copy loop
EMB_SPECS = {
    "row_stride": (2100, 256, (2, 1)),
    "copy_tail_one_thread": (5, 2056, (1, 2)),
    "copy_loop_512": (5, 4096, (1, 2)),
    "grid_at_cap": (2048, 8, (1, 1)),
    "grid_cap_plus_1": (2049, 8, (2, 1)),
}
EMB_V = 300


@dataclass
class EmbCase:
    name: str
    T: int
    H: int
    table: torch.Tensor
    ids: torch.Tensor
    _t: dict = field(default_factory=dict)

    def oracle(self):
        return self.table[self.ids.long()].to(F64)

    def ss64(self):
        return self.oracle().pow(2).sum(-1)

    def cpu_path(self, with_ss=False):
        from agentfield_amd import ops
        ss = torch.full((self.T, 8), float("nan")) if with_ss else None
        return ops.embedding(self.ids, self.table, ss=ss), ss

    def mutant(self, mut: str):
        R = self.oracle().clone()
        if mut == "stride_alias":
            R[ROW_CAP:] = R[:max(0, self.T - ROW_CAP)].clone()
        elif mut == "beyond_cap_unwritten":
            R[ROW_CAP:] = float("nan")
        elif mut == "inner_loop_single_trip":
            R[:, NTHR * 8:] = float("nan")
        else:
            raise ValueError(mut)
        return R


_EMB_CACHE: dict = {}


def emb_case(name: str) -> EmbCase:
    if name not in _EMB_CACHE:
        T, H, _ = EMB_SPECS[name]
        g = gen(8000 + list(EMB_SPECS).index(name))
        table = scaled_rows(g, EMB_V, H).to(BF)
        ids = torch.randint(0, EMB_V, (T,), generator=g)
        ids[1] = ids[0]                       # a repeated id
        ids[2] = EMB_V - 1                    # the last row of the table
        if T > ROW_CAP:                       # rows one cap apart differ
            ids[ROW_CAP:] = (ids[:T - ROW_CAP] + 1) % EMB_V
            ids[T - 1] = EMB_V - 1 if ids[T - 1 - ROW_CAP] != EMB_V - 1 else 0
        _EMB_CACHE[name] = EmbCase(name, T, H, table, ids.to(torch.int32))
    return _EMB_CACHE[name]


# ------------------------------------------------------------- SwiGLU / add
# name -> (T, I, scaled, claimed arm): blocks and trips of the stride loop
SILU_SPECS = {
    "stride_loop_plain": (2100, 2048, False, (2048, 2)),
    "stride_loop_scaled": (2100, 2048, True, (2048, 2)),
    "vectors_at_cap": (2048, 2048, False, (2048, 1)),
    "vectors_cap_plus_row": (2049, 2048, False, (2048, 2)),
    "below_cap": (31, 1024, False, (16, 1)),
}
SILU_MUTANTS = ("stride_alias", "beyond_cap_unwritten", "silu_scale_one_slot")
ADD_N = 8 * (VEC_CAP + 300)       # af_add: 300 vectors make a second trip


@dataclass
class SiluCase:
    name: str
    T: int
    I: int
    gu: torch.Tensor
    ss: torch.Tensor | None
    kdim: int
    _t: dict = field(default_factory=dict)

    @property
    def scale(self):
        return None if self.ss is None else (self.ss, self.kdim, EPS)

    def oracle(self, mut=None):
        if mut not in self._t:
            rstd = None
            if self.ss is not None:
                rstd = rstd64(self.ss, self.kdim, EPS)
                if mut == "silu_scale_one_slot":
                    rstd = torch.rsqrt(self.ss[:, 0].to(F64) / self.kdim + EPS)
            R = swiglu64(self.gu, rstd)
            if mut in ("stride_alias", "beyond_cap_unwritten"):
                flat = R.clone().flatten()
                n = flat.numel() - VEC_CAP * 8
                if n > 0:
                    flat[VEC_CAP * 8:] = (flat[:n].clone() if mut ==
                                          "stride_alias" else float("nan"))
                R = flat.view_as(R)
            self._t[mut] = R
        return self._t[mut]

    def cpu_path(self):
        from agentfield_amd import ops
        if "W" not in self._t:
            self._t["W"] = ops.silu_and_mul(self.gu, scale=self.scale)
        return self._t["W"]


_SILU_CACHE: dict = {}


def silu_case(name: str) -> SiluCase:
    if name not in _SILU_CACHE:
        T, I, scaled, _ = SILU_SPECS[name]
        g = gen(9000 + list(SILU_SPECS).index(name))
        gu = scaled_rows(g, T, 2 * I).to(BF)
        kdim = 256
        ss = ss8(g, gu[:, :kdim]) if scaled else None
        _SILU_CACHE[name] = SiluCase(name, T, I, gu, ss, kdim)
    return _SILU_CACHE[name]


def add_inputs():
    g = gen(9500)
    n_rows = ADD_N // 8
    a = scaled_rows(g, n_rows, 8).to(BF).flatten()
    b = scaled_rows(g, n_rows, 8).to(BF).flatten()
    return a, b


# ------------------------------------------------------------------- gather
GATHER_T = 37
GATHER_IDX = {1: [GATHER_T - 1],
              11: [0, GATHER_T - 1, 5, 5, 20, 1, 36, 8, 13, 21, 2]}
GATHER_BH = [(B, H) for B in (1, 11) for H in (8, 2056, 16384)]


def gather_case(B: int, H: int):
    """x [GATHER_T, H] bf16, idx [B] i32 (a repeat, row 0 and the last row)."""
    g = gen(9700 + B + H)
    return (scaled_rows(g, GATHER_T, H).to(BF),
            torch.tensor(GATHER_IDX[B], dtype=torch.int32))


def gather_mutant(x, idx, mut: str):
    R = x[idx.long()].to(F64)
    assert mut == "inner_loop_single_trip"
    R[:, NTHR * 8:] = float("nan")
    return R


# --------------------------------------------------- one prefill model step
STEP_HISTS = [0] * 9 + [65, 130]
STEP_LENS = [1, 17, 64, 129, 257, 300, 400, 440, 511, 64, 5]


def llama_prefill64(sd, cfg, ids, positions, kcs, vcs, bt, q_start, cu,
                    slots, table, logit_rows=None):
    """fp64 Llama prefill forward (dense, standard path): the prefill twin
    of attn_cases.llama_decode64.  sd: state dict upcast to fp64; kcs/vcs:
    per-layer fp64 caches, updated in place.  Returns logits [T or
    len(logit_rows), V]."""
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
        o = paged_prefill64(q, kcs[i], vcs[i], bt, q_start, cu, scale)
        x = x + o @ sd[p + "attn.o"].t()
        gu = norm(x, sd[p + "post_norm"]) @ sd[p + "mlp.gate_up"].t()
        x = x + swiglu64(gu) @ sd[p + "mlp.down"].t()
    x = norm(x, sd["final_norm"])
    if logit_rows is not None:
        x = x[logit_rows.long()]
    return x @ sd["lm_head"].t()


@dataclass
class PrefillStepCase:
    """One prefill call of CONFIGS["tiny"] (random norm weights, not folded,
    standard path): eleven sequences, two of them chunks that attend to
    cached history, T = 2188 rows."""
    cfg: object
    model: object
    ids: torch.Tensor
    pos: torch.Tensor
    slots: torch.Tensor
    bt: torch.Tensor
    q_start: torch.Tensor
    cu: torch.Tensor
    lens: list
    rows: torch.Tensor         # last row of every sequence
    kcs: list
    vcs: list
    page: int
    _t: dict = field(default_factory=dict)

    @property
    def T(self):
        return int(self.ids.numel())

    def metadata(self, dev="cpu"):
        from agentfield_amd.models.llama import AttnMetadata
        return AttnMetadata(is_prefill=True, slots=self.slots.to(dev),
                            cu_seqlens=self.cu.to(dev),
                            seq_lens=list(self.lens),
                            q_start=self.q_start.to(dev),
                            block_table=self.bt.to(dev))

    def kv(self, dev="cpu"):
        from agentfield_amd.models.llama import KVCache
        kv = KVCache(self.cfg, self.kcs[0].shape[0], self.page, dev)
        for i in range(self.cfg.num_layers):
            kv.k[i].copy_(self.kcs[i])
            kv.v[i].copy_(self.vcs[i])
        return kv

    def oracle(self):
        """(logits [11, V], per-layer fp64 k caches, v caches)."""
        if "T" not in self._t:
            sd = {k: v.to(F64) for k, v in self.model.state_dict().items()}
            kcs = [k.to(F64) for k in self.kcs]
            vcs = [v.to(F64) for v in self.vcs]
            logits = llama_prefill64(
                sd, self.cfg, self.ids, self.pos, kcs, vcs, self.bt,
                self.q_start.tolist(), self.cu.tolist(), self.slots.tolist(),
                self.model.rope_tab, self.rows)
            self._t["T"] = (logits, kcs, vcs)
        return self._t["T"]

    def cpu_path(self):
        """(logits [11, V], the CPU model's KVCache after the call)."""
        if "W" not in self._t:
            kv = self.kv("cpu")
            with torch.no_grad():
                logits = self.model(self.ids, self.pos, kv,
                                    self.metadata("cpu"),
                                    logit_rows=self.rows)
            self._t["W"] = (logits, kv)
        return self._t["W"]


_PSTEP_CACHE: dict = {}


def prefill_step_case(seed: int = 11, page: int = 16) -> PrefillStepCase:
    if "c" in _PSTEP_CACHE:
        return _PSTEP_CACHE["c"]
    from agentfield_amd.models import CONFIGS
    from agentfield_amd.models.llama import LlamaForCausalLM
    cfg = CONFIGS["tiny"]
    g = gen(seed)
    model = LlamaForCausalLM(cfg, device="cpu").init_random(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_((1 + 0.1 * torch.randn(p.shape, generator=g)).to(BF))
    totals = [h + n for h, n in zip(STEP_HISTS, STEP_LENS)]
    assert max(totals) < cfg.max_position
    bt, npages = _pages_for(totals, page, g)
    shape = (npages, cfg.num_kv_heads, page, cfg.head_dim)
    kcs = [randn_bf16(g, *shape, scale=0.3) for _ in range(cfg.num_layers)]
    vcs = [randn_bf16(g, *shape, scale=0.3) for _ in range(cfg.num_layers)]
    T = sum(STEP_LENS)
    ids = torch.randint(0, cfg.vocab_size, (T,), generator=g).to(torch.int32)
    pos, slots, cu = [], [], [0]
    for s, (h, n) in enumerate(zip(STEP_HISTS, STEP_LENS)):
        for p in range(h, h + n):
            pos.append(p)
            slots.append(int(bt[s, p // page]) * page + p % page)
        cu.append(cu[-1] + n)
    cu_t = torch.tensor(cu, dtype=torch.int32)
    c = PrefillStepCase(
        cfg, model, ids, torch.tensor(pos, dtype=torch.int32),
        torch.tensor(slots, dtype=torch.int64), bt,
        torch.tensor(STEP_HISTS, dtype=torch.int32), cu_t, list(STEP_LENS),
        (cu_t[1:] - 1).to(torch.int32), kcs, vcs, page)
    _PSTEP_CACHE["c"] = c
    return c
