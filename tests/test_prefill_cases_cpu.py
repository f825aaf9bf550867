"""CPU-tier adequacy test for the prefill-sized row-kernel cases.

1. Every case runs through the project's own CPU path (``ops.*`` on CPU
   tensors) and is checked against the fp64 oracle, per row.
2. Mutated fp64 oracles (one defect of a launch arm each) must FAIL the GPU
   tests' pass criterion ``row_err <= MARGIN * row_err(W)`` on the case that
   names that arm — a mutant that survives means the case or the row scaling
   is wrong.
3. The fp64 prefill forward agrees with the CPU model.
4. The arm every GPU case claims follows from the kernels' launch rules.

Nothing here is measured against a kernel.
"""
import pytest
import torch

import attn_cases as ac
import prefill_cases as pc
from agentfield_amd import ops

# One rounding of an fp32 result to bf16 (derivation in
# test_attn_cases_cpu.py): half an ulp is at most 2^-8 of the value, hence of
# its row's max|T|; 1% on top for fp32 accumulation moving a value across a
# rounding boundary.
W_BOUND = 2.0 ** -8 * 1.01
W_FLOOR = 2.0 ** -12
# rope_cache with scale: the CPU path rounds rstd, the scaled row and the
# rotated row to bf16 (2^-8 each at most).  A rotated element y1*c - y2*s
# carries the first two errors of both inputs, 2 * 2^-8 * (|y1 c| + |y2 s|)
# <= 2 * sqrt(2) * 2^-8 * max|y|, and its own rounding: (2 sqrt(2) + 1) * 2^-8
# ~ 3.83 * 2^-8 of the row maximum (a rotation keeps the row maximum within a
# few percent over >= 768 elements); 4 * 2^-8 as in test_attn_cases_cpu.py.
W_BOUND_ROPE_SCALED = 4 * 2.0 ** -8
# scaled v rows: the CPU path multiplies by the bf16-rounded rstd and rounds
# the product, two roundings of 2^-8 each.
W_BOUND_V_SCALED = 2 * 2.0 ** -8 * 1.01
# SwiGLU with scale: the CPU path rounds the scaled gate and up (2^-8 each)
# and the result (2^-8).  |silu'| <= 1.1, so the gate's error moves silu(g) by
# at most 1.1 * 2^-8 * |g|; with |silu(g) u| <= |g u| the three terms sum to
# at most 3.1 * 2^-8 * max|g u| of the row, and max|out| ~ max|g u| because
# silu(g) ~ g at the row's largest gates.  4 * 2^-8 leaves that slack.
W_BOUND_SILU_SCALED = 4 * 2.0 ** -8

RMS_KEYS = [(n, r) for n in pc.RMS_SPECS for r in (False, True)]
ROPE_KEYS = [(n, s) for n in pc.ROPE_SPECS for s in (False, True)]


# ---------------------------------------------------- 1. W against the oracle
@pytest.mark.parametrize("name,residual", RMS_KEYS)
def test_rmsnorm_case_cpu_path_matches_oracle(name, residual):
    c = pc.rms_case(name, residual)
    x0 = c.x.clone()
    res0 = None if c.res is None else c.res.clone()
    (out, new_res), (T, h) = c.cpu_path(), c.oracle()
    e = pc.row_err(out, T)
    print(f"rmsnorm {name} res={residual}: row_err(W)={e:.3e}")
    assert W_FLOOR <= e <= W_BOUND, (name, e)
    assert torch.equal(c.x, x0)
    # the tiny row really has mean(h^2) < eps
    assert h[c.tiny_row].pow(2).mean().item() < pc.EPS
    if residual:
        assert torch.equal(c.res, res0), "the case's inputs stay unchanged"
        # bf16(x + res): one correctly rounded fp32 add, RNE to bf16
        assert torch.equal(new_res, (c.x.float() + c.res.float()).to(ac.BF))
        assert pc.row_err(new_res, h) <= W_BOUND


@pytest.mark.parametrize("name,scaled", ROPE_KEYS)
def test_rope_case_cpu_path_matches_oracle(name, scaled):
    c = pc.rope_case(name, scaled)
    Wv, Tv = c.views(c.cpu_path()), c.views(c.oracle())
    bound = W_BOUND_ROPE_SCALED if scaled else W_BOUND
    for n in ("q", "k", "kc_rows"):
        e = pc.row_err(Wv[n], Tv[n])
        print(f"rope {name} scaled={scaled} {n}: row_err(W)={e:.3e}")
        assert W_FLOOR <= e <= bound, (name, n, e)
    ev = pc.row_err(Wv["vc_rows"], Tv["vc_rows"])
    if scaled:
        assert W_FLOOR <= ev <= W_BOUND_V_SCALED, (name, ev)
    else:
        assert ev == 0.0
    for n in ("kc_rest", "vc_rest"):
        assert torch.equal(Wv[n].to(ac.F64), Tv[n])
    assert int(c.pos.max()) == pc.ROPE_MAX_POS - 1
    assert c.skip.any() and (~c.skip).any()
    assert c.qkv[:, c.sl[0]].stride(0) != c.qkv[:, c.sl[0]].shape[1]


@pytest.mark.parametrize("name", list(pc.CACHE_SPECS))
def test_cache_case_cpu_path_matches_oracle(name):
    c = pc.cache_case(name)
    W, T = c.cpu_path(), c.oracle()
    for n in ("kc", "vc"):
        assert torch.equal(W[n].to(ac.F64), T[n]), "a scatter is a pure copy"
    assert c.killed(W) == 0.0


@pytest.mark.parametrize("name", list(pc.EMB_SPECS))
def test_embedding_case_cpu_path_matches_oracle(name):
    c = pc.emb_case(name)
    out, ss = c.cpu_path(with_ss=True)
    assert torch.equal(out.to(ac.F64), c.oracle())
    assert torch.equal(ss[:, 1:], torch.zeros(c.T, 7))
    rel = ((ss[:, 0].to(ac.F64) - c.ss64()).abs() / c.ss64()).max().item()
    assert rel <= (c.H + 2) * 2.0 ** -24
    ids = c.ids.tolist()
    assert len(set(ids)) < len(ids) and pc.EMB_V - 1 in ids


@pytest.mark.parametrize("name", list(pc.SILU_SPECS))
def test_silu_case_cpu_path_matches_oracle(name):
    c = pc.silu_case(name)
    e = pc.row_err(c.cpu_path(), c.oracle())
    print(f"silu {name}: row_err(W)={e:.3e}")
    bound = W_BOUND_SILU_SCALED if c.ss is not None else W_BOUND
    assert W_FLOOR <= e <= bound, (name, e)
    if c.ss is not None:      # eight distinct slots
        assert (c.ss.sort(-1).values.diff(dim=-1) > 0).all()


@pytest.mark.parametrize("B,H", pc.GATHER_BH)
def test_gather_case(B, H):
    x, idx = pc.gather_case(B, H)
    got = ops.gather_rows(x, idx)
    assert torch.equal(got, x[idx.long()])
    il = idx.tolist()
    assert pc.GATHER_T - 1 in il
    if B > 1:
        assert 0 in il and len(set(il)) < len(il)


# ------------------------------------------------------------- 2. the mutants
def _rms_kill(name, residual, mut, wave=0):
    c = pc.rms_case(name, residual)
    (W, _), (T, _), (M, _) = c.cpu_path(), c.oracle(), c.oracle(mut, wave)
    return pc.exceeds_budget(M, W, T), pc.kill_ratio(M, W, T)


# mutant -> the cases named for the arm it breaks
RMS_KILLERS = {
    "stride_alias": ["block_row_stride", "block_row_stride_3trips"],
    "beyond_cap_unwritten": ["block_row_stride", "block_row_stride_3trips"],
    "neighbour_stat": ["block_thread0_only", "block_one_full_iter",
                       "block_eight_full_iters", "block_step_shape"],
    "tail_iter_dropped": ["block_tail_one_thread"],
    "tail_iter_sum_dropped": ["block_tail_one_thread"],
    "eps_outside": list(pc.RMS_SPECS),
    "residual_not_added": list(pc.RMS_SPECS),
}


@pytest.mark.parametrize("mut", list(RMS_KILLERS))
def test_rmsnorm_mutant_is_killed(mut):
    for name in RMS_KILLERS[mut]:
        for residual in ((True,) if mut == "residual_not_added"
                         else (False, True)):
            dead, ratio = _rms_kill(name, residual, mut)
            print(f"rmsnorm mutant {mut}: {name} res={residual} "
                  f"kill ratio {ratio:.1f}")
            assert dead, (mut, name, residual, ratio)


@pytest.mark.parametrize("wave", [0, 1, 2, 3])
def test_rmsnorm_wave_partial_dropped_is_killed(wave):
    """Each of the four red[] partials, on the cases where every wave holds
    columns."""
    for name in ("block_one_full_iter", "block_eight_full_iters"):
        for residual in (False, True):
            dead, ratio = _rms_kill(name, residual, "wave_partial_dropped",
                                    wave)
            print(f"rmsnorm mutant wave_partial_dropped[{wave}]: {name} "
                  f"res={residual} kill ratio {ratio:.1f}")
            assert dead, (wave, name, residual, ratio)


def test_rmsnorm_residual_not_updated_is_killed():
    for name in pc.RMS_SPECS:
        c = pc.rms_case(name, True)
        (_, new_res), (_, h) = c.cpu_path(), c.oracle()
        assert pc.exceeds_budget(c.res, new_res, h), name
        print(f"rmsnorm mutant residual_not_updated: {name} kill ratio "
              f"{pc.kill_ratio(c.res, new_res, h):.1f}")
        assert not torch.equal(c.res, new_res)


ROW_KILLERS = {
    "stride_alias": ["row_stride"],
    "beyond_cap_unwritten": ["row_stride"],
}


@pytest.mark.parametrize("mut", pc.ROW_MUTANTS)
def test_rope_mutant_is_killed(mut):
    names = ROW_KILLERS.get(mut, ["rot_loop_640", "rot_loop_1024_vcopy_512"])
    for name in names:
        for scaled in (False, True):
            c = pc.rope_case(name, scaled)
            ratio = c.killed(c.mutant(mut))
            print(f"rope mutant {mut}: {name} scaled={scaled} "
                  f"kill ratio {ratio:.1f}")
            assert ratio > ac.MARGIN, (mut, name, scaled)
            assert c.killed(c.oracle()) == 0.0


def test_rope_vcopy_single_trip_is_killed_by_v_alone():
    """With Hk = 32 the v copy makes a second trip: a kernel that stops
    after one leaves kv heads 16..31 of the v cache unwritten."""
    c = pc.rope_case("rot_loop_1024_vcopy_512", False)
    R = {n: t.clone() for n, t in c.oracle().items()}
    M = c.mutant("inner_loop_single_trip")
    R["vc"] = M["vc"]
    assert c.killed(R) > ac.MARGIN


@pytest.mark.parametrize("mut", pc.ROW_MUTANTS)
def test_cache_mutant_is_killed(mut):
    name = ROW_KILLERS.get(mut, ["copy_loop_512"])[0]
    c = pc.cache_case(name)
    ratio = c.killed(c.mutant(mut))
    print(f"cache mutant {mut}: {name} kill ratio {ratio}")
    assert ratio > ac.MARGIN, (mut, name)


@pytest.mark.parametrize("mut", pc.ROW_MUTANTS)
def test_embedding_mutant_is_killed(mut):
    names = ROW_KILLERS.get(mut, ["copy_tail_one_thread", "copy_loop_512"])
    if mut != "inner_loop_single_trip":
        names = names + ["grid_cap_plus_1"]
    for name in names:
        c = pc.emb_case(name)
        W, T, M = c.cpu_path()[0], c.oracle(), c.mutant(mut)
        print(f"embedding mutant {mut}: {name} kill ratio "
              f"{pc.kill_ratio(M, W, T)}")
        assert pc.exceeds_budget(M, W, T), (mut, name)
    # the case one row short of the second trip is blind to it, as it must be
    c = pc.emb_case("grid_at_cap")
    assert not pc.exceeds_budget(c.mutant(mut), c.cpu_path()[0], c.oracle())


@pytest.mark.parametrize("mut", pc.SILU_MUTANTS)
def test_silu_mutant_is_killed(mut):
    if mut == "silu_scale_one_slot":
        names = ["stride_loop_scaled"]
    else:
        names = ["stride_loop_plain", "stride_loop_scaled",
                 "vectors_cap_plus_row"]
    for name in names:
        c = pc.silu_case(name)
        W, T, M = c.cpu_path(), c.oracle(), c.oracle(mut)
        print(f"silu mutant {mut}: {name} kill ratio "
              f"{pc.kill_ratio(M, W, T):.1f}")
        assert pc.exceeds_budget(M, W, T), (mut, name)


@pytest.mark.parametrize("B,H", [(B, H) for B, H in pc.GATHER_BH if H > 2048])
def test_gather_mutant_is_killed(B, H):
    x, idx = pc.gather_case(B, H)
    W = ops.gather_rows(x, idx)
    M = pc.gather_mutant(x, idx, "inner_loop_single_trip")
    assert pc.exceeds_budget(M, W, W.to(ac.F64)), (B, H)


def test_row_err_sees_what_the_global_error_hides():
    """A small row that is 3% off: invisible to err, visible to row_err."""
    g = ac.gen(1)
    T = (pc.scaled_rows(g, 14, 64)).to(ac.F64)
    W = T.float().to(ac.BF)
    M = T.clone()
    M[0] *= 1.03                       # row 0 has scale 2^-3, row 6 2^3
    assert not ac.exceeds_budget(M, W, T)
    assert pc.exceeds_budget(M, W, T)
    Z = torch.zeros(2, 4, dtype=ac.F64)
    assert pc.row_err(Z + 0.5, Z) == 0.5     # max|T| = 0: absolute error
    assert pc.exceeds_budget(torch.full((2, 4), float("nan")), Z, Z)


# --------------------------------------------------- 3. the step oracle
def test_prefill_step_oracle_matches_cpu_model():
    """fp64 Llama prefill forward vs the CPU model (standard path)."""
    c = pc.prefill_step_case()
    assert c.T == 2188 and c.rows.numel() == 11
    (Wl, kv), (Tl, kcs, vcs) = c.cpu_path(), c.oracle()
    e = ac.err(Wl, Tl)
    print(f"prefill step: err(W) logits={e:.3e}")
    # as in test_step_oracle_matches_cpu_model: ~20 bf16 roundings between
    # embedding and logits, each <= 2^-9 of its tensor's scale, which do not
    # all align; 2^-5 is a loose ceiling that a wrong oracle (O(1) error)
    # cannot meet.  The cache rows of layer i sit behind 3 + 10 i of those
    # roundings (norm, qkv GEMM, rope), so the same ceiling holds for them.
    assert 0 < e <= 2.0 ** -5
    w = c.slots
    for i in range(c.cfg.num_layers):
        for got, truth, init, tag in ((kv.k[i], kcs[i], c.kcs[i], "k"),
                                      (kv.v[i], vcs[i], c.vcs[i], "v")):
            ec = ac.err(pc.slot_rows(got, w), pc.slot_rows(truth, w))
            print(f"prefill step: err(W) layer {i} {tag} cache={ec:.3e}")
            assert 0 < ec <= 2.0 ** -5
            assert torch.equal(pc.rest_of(got, w), pc.rest_of(init, w))
            assert torch.equal(pc.rest_of(truth, w),
                               pc.rest_of(init, w).to(ac.F64))


# ------------------------------------------------------ 4. the arms claimed
def test_rmsnorm_arms():
    for name, (T, H, (arm, its, last, trips)) in pc.RMS_SPECS.items():
        assert pc.rmsnorm_arm(T) == arm, name
        assert pc.rmsnorm_iters(H) == (its, last), name
        assert pc.grid_rows(T, pc.RMS_CAP)[1] == trips, name
        assert H % 8 == 0 and H <= 16384
    Ts = {T for T, _, _ in pc.RMS_SPECS.values()}
    assert {256, 257} <= Ts                      # both sides of the dispatch
    assert pc.rmsnorm_arm(256) == "wave" and pc.rmsnorm_arm(257) == "block"
    assert pc.grid_rows(16384, pc.RMS_CAP) == (16384, 1)
    assert pc.grid_rows(16385, pc.RMS_CAP) == (16384, 2)
    assert pc.rmsnorm_iters(16384) == (8, 256)   # the supported maximum
    assert pc.rmsnorm_iters(2048) == (1, 256)
    assert pc.rmsnorm_iters(2056) == (2, 1)


def test_row_kernel_arms():
    for name, (T, Hq, Hk, (rows, rot, vcp)) in pc.ROPE_SPECS.items():
        assert pc.grid_rows(T, pc.ROW_CAP)[1] == rows, name
        assert pc.inner_trips(pc.rope_work(Hq, Hk)) == rot, name
        assert pc.inner_trips(pc.vcopy_work(Hk)) == vcp, name
    assert pc.rope_work(32, 8) == 640 and pc.rope_work(32, 32) == 1024
    assert pc.vcopy_work(32) == 512
    for name, (T, Hk, (rows, cp)) in pc.CACHE_SPECS.items():
        assert pc.grid_rows(T, pc.ROW_CAP)[1] == rows, name
        assert pc.inner_trips(pc.vcopy_work(Hk)) == cp, name
    for name, (T, H, (rows, cp)) in pc.EMB_SPECS.items():
        assert pc.grid_rows(T, pc.ROW_CAP)[1] == rows, name
        assert pc.inner_trips(pc.embed_work(H)) == cp, name
    assert pc.grid_rows(2048, pc.ROW_CAP) == (2048, 1)
    assert pc.grid_rows(2049, pc.ROW_CAP) == (2048, 2)
    Ts = {T for T, _, _ in pc.EMB_SPECS.values()}
    assert {2048, 2049} <= Ts
    assert pc.inner_trips(256) == 1 and pc.inner_trips(257) == 2
    for _, H in pc.GATHER_BH:
        assert pc.gather_trips(H) == {8: 1, 2056: 2, 16384: 8}[H]
    assert pc.gather_trips(2048) == 1 and pc.gather_trips(2049) == 2
    c = pc.prefill_step_case()
    assert pc.grid_rows(c.T, pc.ROW_CAP)[1] == 2
    assert pc.rmsnorm_arm(c.T) == "block"


def test_vector_kernel_arms():
    for name, (T, I, _, arm) in pc.SILU_SPECS.items():
        assert pc.silu_blocks(T, I) == arm, name
    nv = {T * (I >> 3) for T, I, _, _ in pc.SILU_SPECS.values()}
    assert pc.VEC_CAP in nv                       # exactly one full trip
    assert any(pc.VEC_CAP < n <= pc.VEC_CAP + 256 for n in nv)
    assert pc.vec_blocks(pc.VEC_CAP) == (2048, 1)
    assert pc.vec_blocks(pc.VEC_CAP + 1) == (2048, 2)
    assert pc.vec_blocks(pc.VEC_CAP - 256 + 1) == (2048, 1)
    assert pc.vec_blocks(pc.VEC_CAP - 256) == (2047, 1)
    assert pc.vec_blocks(pc.ADD_N // 8) == (2048, 2)
