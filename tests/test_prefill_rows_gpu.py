"""The prefill-sized arms of the row kernels against fp64: RMSNorm (block
kernel, partial last iteration, row stride), RoPE + cache append, cache
scatter, embedding, SwiGLU, add and row gather beyond their grid caps and
with inner loops that make a second trip, and one prefill step of the model
(cases, oracles and criterion in tests/prefill_cases.py).

Criterion per tensor: row_err(K) <= 4 * row_err(W); pure copies and single
correctly-rounded fp32 operations are bit-exact.  Outputs a kernel might skip
are caller-allocated and pre-filled with NaN.
"""
import pytest
import torch

import attn_cases as ac
import prefill_cases as pc
from agentfield_amd import ops
from agentfield_amd.ops import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = pc.EPS

RMS_KEYS = [(n, r) for n in pc.RMS_SPECS for r in (False, True)]
ROPE_KEYS = [(n, s) for n in pc.ROPE_SPECS for s in (False, True)]
_TAB: dict = {}


def _tab():
    if "t" not in _TAB:
        _TAB["t"] = pc.rope_tab().to(DEV)
    return _TAB["t"]


def _finite(t: torch.Tensor, what: str):
    assert torch.isfinite(t.float()).all(), f"{what}: NaN pre-fill survives"


# ------------------------------------------------------------------ rmsnorm
@pytest.mark.parametrize("name,residual", RMS_KEYS)
def test_rmsnorm_arm(name, residual):
    c = pc.rms_case(name, residual)
    T, H, (arm, its, last, trips) = pc.RMS_SPECS[name]
    assert pc.rmsnorm_arm(T) == arm
    x, w = c.x.to(DEV), c.w.to(DEV)
    res = c.res.to(DEV) if residual else None
    out = pc.nan_bf16(T, H).to(DEV)
    rc = _lib.lib().af_rmsnorm(_lib.ptr(out), _lib.ptr(res), _lib.ptr(x),
                               _lib.ptr(res), _lib.ptr(w), EPS, T, H,
                               _lib.cur_stream())
    _lib.check(rc, "af_rmsnorm")
    torch.cuda.synchronize()
    out = out.cpu()
    _finite(out, "rmsnorm out")
    (Wout, Wres), (T64, _) = c.cpu_path(), c.oracle()
    pc.row_budget_check(
        f"rmsnorm {name} T={T} H={H} res={residual} [{arm}, {its} iter, "
        f"{last} threads in the last, {trips} row trips]", out, Wout, T64)
    assert torch.equal(x.cpu(), c.x), "x must stay unchanged"
    if residual:
        assert torch.equal(res.cpu(), Wres), "new residual = bf16(x + res)"
        res2 = c.res.to(DEV)
        out2, new = ops.rmsnorm(x, w, EPS, residual=res2)
        torch.cuda.synchronize()
        assert new is res2 or new.data_ptr() == res2.data_ptr(), \
            "the residual is updated in the storage that was passed in"
        assert torch.equal(new.cpu(), Wres)
    else:
        out2 = ops.rmsnorm(x, w, EPS)
        torch.cuda.synchronize()
    assert torch.equal(out2.cpu(), out)


def test_rmsnorm_rejects_unsupported_H_and_accepts_T0():
    for H in (16392, 12):      # > 16384; not a multiple of 8
        x = torch.zeros(4, H, dtype=ac.BF, device=DEV)
        w = torch.ones(H, dtype=ac.BF, device=DEV)
        with pytest.raises(ops.AfOpsError):
            ops.rmsnorm(x, w, EPS)
        with pytest.raises(ops.AfOpsError):
            ops.rmsnorm(x, w, EPS, residual=torch.zeros_like(x))
    x = torch.zeros(0, 256, dtype=ac.BF, device=DEV)
    w = torch.ones(256, dtype=ac.BF, device=DEV)
    assert ops.rmsnorm(x, w, EPS).shape == (0, 256)
    out, res = ops.rmsnorm(x, w, EPS, residual=torch.zeros_like(x))
    torch.cuda.synchronize()
    assert out.shape == (0, 256) and res.shape == (0, 256)


# ----------------------------------------------- rope + cache / cache only
def _check_cache_case(c, K, tag):
    Kv, Wv, Tv = (c.views(r) for r in (K, c.cpu_path(), c.oracle()))
    w = c.written
    for n, init in (("kc_rest", c.kc0), ("vc_rest", c.vc0)):
        assert torch.equal(Kv[n], pc.rest_of(init, w)), \
            f"{tag}: untouched {n[:2]} slots changed"
    names = ["q", "k"] if c.rope else []
    for n in names + ["kc_rows", "vc_rows"]:
        pc.row_budget_check(f"{tag} {n}", Kv[n], Wv[n], Tv[n])
    if not c.scaled:           # v rows (and k rows without rope): pure copy
        assert torch.equal(Kv["vc_rows"], Wv["vc_rows"])
        assert torch.equal(Kv["vc_rows"].to(ac.F64), Tv["vc_rows"])
    if not c.rope:
        assert torch.equal(Kv["kc_rows"], Wv["kc_rows"])


@pytest.mark.parametrize("name,scaled", ROPE_KEYS)
def test_rope_cache_arm(name, scaled):
    c = pc.rope_case(name, scaled)
    T, Hq, Hk, (rows, rot, vcp) = pc.ROPE_SPECS[name]
    qkv, kc, vc = (t.clone().to(DEV) for t in (c.qkv, c.kc0, c.vc0))
    q, k, v = (qkv[:, s] for s in c.sl)
    assert q.stride(0) != q.shape[1]
    ops.rope_cache(q, k, v, c.pos.to(DEV), _tab(), kc, vc, c.slots.to(DEV),
                   scale=c.scale(c.ss.to(DEV) if scaled else None))
    torch.cuda.synchronize()
    assert torch.equal(v.cpu(), c.qkv[:, c.sl[2]]), "v rows are read-only"
    K = dict(q=q.cpu(), k=k.cpu(), kc=kc.cpu(), vc=vc.cpu())
    _check_cache_case(
        c, K, f"rope-cache {name} T={T} Hq={Hq} Hk={Hk} "
        f"{'scaled' if scaled else 'plain'} [{rows} row trips, {rot} rotation "
        f"trips, {vcp} v-copy trips]")


@pytest.mark.parametrize("name", list(pc.CACHE_SPECS))
def test_reshape_and_cache_arm(name):
    c = pc.cache_case(name)
    T, Hk, (rows, cp) = pc.CACHE_SPECS[name]
    _, sk, sv = c.sl
    k = c.qkv[:, sk].unflatten(-1, (Hk, ac.D)).contiguous().to(DEV)
    v = c.qkv[:, sv].unflatten(-1, (Hk, ac.D)).contiguous().to(DEV)
    kc, vc = c.kc0.clone().to(DEV), c.vc0.clone().to(DEV)
    ops.reshape_and_cache(k, v, kc, vc, c.slots.to(DEV))
    torch.cuda.synchronize()
    _check_cache_case(c, dict(kc=kc.cpu(), vc=vc.cpu()),
                      f"reshape-and-cache {name} T={T} Hk={Hk} "
                      f"[{rows} row trips, {cp} copy trips]")


# ---------------------------------------------------------------- embedding
@pytest.mark.parametrize("with_ss", [False, True])
@pytest.mark.parametrize("name", list(pc.EMB_SPECS))
def test_embedding_arm(name, with_ss):
    c = pc.emb_case(name)
    T, H, (rows, cp) = pc.EMB_SPECS[name]
    table, ids = c.table.to(DEV), c.ids.to(DEV)
    out = pc.nan_bf16(T, H).to(DEV)
    ss = torch.full((T, 8), float("nan"), device=DEV) if with_ss else None
    rc = _lib.lib().af_embedding(_lib.ptr(out), _lib.ptr(table),
                                 _lib.ptr(ids), _lib.ptr(ss), T, H,
                                 _lib.cur_stream())
    _lib.check(rc, "af_embedding")
    torch.cuda.synchronize()
    out = out.cpu()
    _finite(out, "embedding out")
    W = c.cpu_path()[0]
    pc.row_budget_check(f"embedding {name} T={T} H={H} ss={with_ss} "
                        f"[{rows} row trips, {cp} copy trips]", out, W,
                        c.oracle())
    assert torch.equal(out, W), "rows must be exact"
    if with_ss:
        ss = ss.cpu()
        assert torch.equal(ss[:, 1:], torch.zeros(T, 7)), "ss[:,1:] must be 0"
        # fp32 sum of H exact products, all positive, every add within
        # 2^-24 relative (test_embedding_with_stats)
        T64 = c.ss64()
        rel = ((ss[:, 0].to(ac.F64) - T64).abs() / T64).max().item()
        print(f"embedding-ss {name}: rel {rel:.3e}")
        assert rel <= (H + 2) * 2.0 ** -24


# ------------------------------------------------------------- SwiGLU / add
@pytest.mark.parametrize("name", list(pc.SILU_SPECS))
def test_silu_and_mul_arm(name):
    c = pc.silu_case(name)
    T, I, scaled, (blocks, trips) = pc.SILU_SPECS[name]
    gu = c.gu.to(DEV)
    out = pc.nan_bf16(T, I).to(DEV)
    ss = c.ss.to(DEV) if scaled else None
    rc = _lib.lib().af_silu_mul(
        _lib.ptr(out), _lib.ptr(gu), _lib.ptr(ss),
        1.0 / c.kdim if scaled else 0.0, EPS if scaled else 0.0, T, I,
        _lib.cur_stream())
    _lib.check(rc, "af_silu_mul")
    torch.cuda.synchronize()
    out = out.cpu()
    _finite(out, "silu_and_mul out")
    pc.row_budget_check(
        f"silu-mul {name} T={T} I={I} {'scaled' if scaled else 'plain'} "
        f"[{T * I // 8} vectors, {blocks} blocks, {trips} stride trips]",
        out, c.cpu_path(), c.oracle())
    assert torch.equal(gu.cpu(), c.gu)


def test_add_stride_loop():
    a, b = pc.add_inputs()
    n = pc.ADD_N
    assert a.numel() == n and pc.vec_blocks(n // 8) == (2048, 2)
    ad, bd = a.to(DEV), b.to(DEV)
    out = pc.nan_bf16(n).to(DEV)
    rc = _lib.lib().af_add(_lib.ptr(out), _lib.ptr(ad), _lib.ptr(bd), n,
                           _lib.cur_stream())
    _lib.check(rc, "af_add")
    torch.cuda.synchronize()
    out = out.cpu()
    _finite(out, "add out")
    W = (a.float() + b.float()).to(ac.BF)
    pc.row_budget_check(f"add n={n} [{n // 8} vectors, 2048 blocks, 2 stride "
                        "trips]", out.view(-1, 8), W.view(-1, 8),
                        (a.to(ac.F64) + b.to(ac.F64)).view(-1, 8))
    assert torch.equal(out, W), "one fp32 add, RNE to bf16"
    assert torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b)


# ------------------------------------------------------------------- gather
@pytest.mark.parametrize("B,H", pc.GATHER_BH)
def test_gather_rows_arm(B, H):
    x, idx = pc.gather_case(B, H)
    xd, idxd = x.to(DEV), idx.to(DEV)
    out = pc.nan_bf16(B, H).to(DEV)
    rc = _lib.lib().af_gather_rows(_lib.ptr(out), _lib.ptr(xd),
                                   _lib.ptr(idxd), B, H, _lib.cur_stream())
    _lib.check(rc, "af_gather_rows")
    torch.cuda.synchronize()
    out = out.cpu()
    _finite(out, "gather_rows out")
    W = x[idx.long()]
    pc.row_budget_check(f"gather-rows B={B} H={H} [{pc.gather_trips(H)} copy "
                        "trips]", out, W, W.to(ac.F64))
    assert torch.equal(out, W)
    assert torch.equal(ops.gather_rows(xd, idxd).cpu(), W)


# --------------------------------------------------- one prefill model step
def test_prefill_step_vs_fp64():
    """One prefill call of CONFIGS["tiny"] (standard path, norms not folded)
    with T = 2188 rows: more than 2048 for embedding and rope_cache, more
    than 256 for rmsnorm; two of the eleven sequences are chunks that attend
    to cached history.

    Logits and, per layer, the K/V cache rows written go through
    budget_check against fp64 and the CPU model; every other cache slot keeps
    its bits.  A second run without logit_rows, indexed afterwards, must give
    the same bits on the last rows: that pins gather_rows inside the model."""
    from agentfield_amd.models.llama import LlamaForCausalLM
    c = pc.prefill_step_case()
    model = LlamaForCausalLM(c.cfg, device=DEV)
    model.load_state_dict(c.model.state_dict())
    (Tl, kcs64, vcs64), (Wl, kvw) = c.oracle(), c.cpu_path()
    ids, pos, md = c.ids.to(DEV), c.pos.to(DEV), c.metadata(DEV)
    rows = c.rows.to(DEV)
    kv = c.kv(DEV)
    with torch.no_grad():
        logits = model(ids, pos, kv, md, logit_rows=rows)
    torch.cuda.synchronize()
    assert logits.shape == (11, c.cfg.vocab_size)
    arm = (f"T={c.T}: rmsnorm {pc.rmsnorm_arm(c.T)}, "
           f"{pc.grid_rows(c.T, pc.ROW_CAP)[1]} row trips")
    ac.budget_check(f"prefill-step logits [{arm}]", logits.cpu(), Wl, Tl)
    w = c.slots
    for i in range(c.cfg.num_layers):
        for got, cpu, truth, init, tag in (
                (kv.k[i].cpu(), kvw.k[i], kcs64[i], c.kcs[i], "k"),
                (kv.v[i].cpu(), kvw.v[i], vcs64[i], c.vcs[i], "v")):
            ac.budget_check(f"prefill-step layer {i} {tag} cache [{arm}]",
                            pc.slot_rows(got, w), pc.slot_rows(cpu, w),
                            pc.slot_rows(truth, w))
            assert torch.equal(pc.rest_of(got, w), pc.rest_of(init, w)), \
                f"layer {i}: untouched {tag} slots changed"
    kv2 = c.kv(DEV)
    with torch.no_grad():
        full = model(ids, pos, kv2, md)
    torch.cuda.synchronize()
    assert full.shape == (c.T, c.cfg.vocab_size)
    picked = full[rows.long()].cpu()
    nd = int((picked != logits.cpu()).sum())
    print(f"prefill-step: logit_rows vs indexing afterwards: {nd} of "
          f"{picked.numel()} logits differ")
    assert torch.equal(picked, logits.cpu()), \
        "gather_rows inside the model picks other rows than indexing does"
