"""Packed grammar token masks on the GPU: the MASKED sampler kernels, the
in-place logit mask, and grammar-constrained decode replayed from a
hipGraph.

Op tests use B=5 and V in {1000, 128256}.  V=1000 gives chunk =
ceil(V/16) = 63, so the sampler's split boundaries fall inside mask words
and V % 32 != 0."""
import functools
import json

import pytest
import torch

from agentfield_amd import ops
from agentfield_amd.engine import LLMEngine, SamplingParams
from agentfield_amd.models import CONFIGS

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 5
VS = (1000, 128256)
SPLITS = 16


@functools.lru_cache(maxsize=None)
def _case(V):
    """(logits bf16 [B,V] on the GPU, its fp32 CPU copy, 50%-density
    membership [B,V] on the CPU).  Shared and never written to."""
    g = torch.Generator().manual_seed(V)
    lf = (torch.randn(B, V, generator=g) * 3.0).to(torch.bfloat16)
    member = torch.rand(B, V, generator=g) < 0.5
    return lf.to(DEV), lf.float(), member


def _pack(member):
    V = member.shape[1]
    return torch.stack([ops.pack_token_mask(m, V) for m in member]).to(DEV)


def _first_argmax(lf, member):
    """Lowest index attaining the maximum over the member set: the
    sampler's documented tie-break."""
    masked = lf.masked_fill(~member, float("-inf"))
    mx = masked.max(-1, keepdim=True).values
    return [int((row == m).nonzero()[0]) for row, m in zip(masked, mx)]


def _sample(logits, temps, st, **kw):
    t = ops.sample(logits, temps, st, **kw)
    torch.cuda.synchronize()
    return t.cpu().tolist()


# ------------------------------------------------------------------ 1. greedy
@pytest.mark.parametrize("V", VS)
def test_masked_greedy(V):
    logits, lf, member = _case(V)
    member = member.clone()
    chunk = (V + SPLITS - 1) // SPLITS
    edge = 7 * chunk                       # first token of split 7
    gmax = int(lf[0].argmax())
    member[0, gmax] = False                # row 0: global argmax disallowed
    for b, only in ((1, 0), (2, V - 1), (3, edge - 1), (4, edge)):
        member[b] = False
        member[b, only] = True
    st = ops.SamplerState(B, DEV)
    temps = torch.zeros(B, dtype=torch.float32, device=DEV)
    got = _sample(logits, temps, st, allowed=_pack(member))
    want = _first_argmax(lf, member)
    assert got == want
    assert got[1:] == [0, V - 1, edge - 1, edge]
    assert got[0] != gmax
    # all ones == no mask
    ones = torch.full((B, (V + 31) // 32), -1, dtype=torch.int32, device=DEV)
    assert _sample(logits, temps, st, allowed=ones) == \
        _sample(logits, temps, st)
    # a row with no bit set yields token 0 (defined behaviour), also at
    # temperature > 0; its neighbours are untouched
    member[0] = False
    assert _sample(logits, temps, st, allowed=_pack(member)) == [0] + want[1:]
    member[4] = False
    hot = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.9], device=DEV)
    assert _sample(logits, hot, st, allowed=_pack(member)) == \
        [0] + want[1:4] + [0]


# ------------------------------------------------------ 2. Gumbel equivalence
@pytest.mark.parametrize("V", VS)
def test_masked_gumbel_equals_additive_mask(V):
    """The masked call on the raw logits draws exactly what the unmasked
    call draws on logits + (-1e30 where disallowed) in bf16 — the path the
    engine used before the bitmask — so the sampler's law carries over."""
    logits, lf, member = _case(V)
    member = member.clone()
    member[3] = False                      # a sparse row: 3 legal tokens,
    member[3, [5, 6, V - 2]] = True        # most splits hold none
    add = torch.zeros(B, V).masked_fill(~member, -1e30).to(torch.bfloat16)
    dense = logits + add.to(DEV)
    allowed = _pack(member)
    temps = torch.tensor([0.0, 0.5, 1.0, 1.0, 1.7], device=DEV)
    sa = ops.SamplerState(B, DEV, seed=1234)
    sb = ops.SamplerState(B, DEV, seed=1234)
    seen = set()
    for step in range(8):
        got = _sample(logits, temps, sa, allowed=allowed)
        want = _sample(dense, temps, sb)
        assert got == want, step
        for b, t in enumerate(got):
            assert member[b, t], (step, b, t)
        seen.add(tuple(got))
    assert len(seen) > 1                   # fresh draws every step
    assert int(sa.step) == int(sb.step) == 8


# -------------------------------------------------------------- 3. top-k/top-p
@pytest.mark.parametrize("V", VS)
def test_masked_topk_topp(V):
    logits, lf, member = _case(V)
    lf, member = lf.clone(), member.clone()
    # a unique allowed maximum per row, so top_k=1 has one answer
    # (randn * 3 stays far below 20)
    top = [int(member[b].nonzero()[int(member[b].sum()) // 3])
           for b in range(B)]
    for b in range(B):
        lf[b, top[b]] = 20.0
    # row 2: every disallowed token sits 30+ above every allowed one
    lf[2][~member[2]] = lf[2][~member[2]].abs() + 50.0
    lf = lf.to(torch.bfloat16).float()
    logits = lf.to(torch.bfloat16).to(DEV)
    assert float(lf[2][~member[2]].min()) >= 50.0
    assert float(lf.masked_fill(~member, -1e9).max()) == 20.0
    allowed = _pack(member)
    st = ops.SamplerState(B, DEV)
    temps = torch.ones(B, dtype=torch.float32, device=DEV)
    topp = torch.ones(B, dtype=torch.float32, device=DEV)
    topk1 = torch.ones(B, dtype=torch.int32, device=DEV)
    got = _sample(logits, temps, st, topk=topk1, topp=topp, allowed=allowed)
    assert got == top == _first_argmax(lf, member)
    # top_k=8: every draw is allowed and at or above the lower edge of the
    # histogram bin holding the 8th-largest ALLOWED logit (span 20 below
    # the ALLOWED max, 256 bins)
    masked = lf.masked_fill(~member, float("-inf"))
    k8 = masked.topk(8, dim=-1).values[:, -1]
    mx = masked.max(-1).values
    gran = 20.0 / 256
    floor8 = torch.floor((k8 - (mx - 20.0)) / gran) * gran + (mx - 20.0)
    topk8 = torch.full((B,), 8, dtype=torch.int32, device=DEV)
    for _ in range(10):
        got = _sample(logits, temps, st, topk=topk8, topp=topp,
                      allowed=allowed)
        for b, t in enumerate(got):
            assert member[b, t], f"row {b} drew disallowed token {t}"
            assert lf[b, t] >= floor8[b] - 1e-3, \
                f"draw below top-8 threshold (b={b}): {lf[b, t]} < {floor8[b]}"
    # a row with no bit set terminates and yields 0, for both threshold arms
    member[4] = False
    allowed = _pack(member)
    for tk in (topk8, topk1):
        got = _sample(logits, temps, st, topk=tk, topp=topp, allowed=allowed)
        assert got[4] == 0
        assert all(member[b, got[b]] for b in range(4))


# ------------------------------------------------------------ 4. mask_logits_
def _bits_equal(a, b):
    return torch.equal(a.view(torch.int16).cpu(), b.view(torch.int16).cpu())


@pytest.mark.parametrize("V", VS)
def test_mask_logits(V):
    logits, lf, member = _case(V)
    member = member.clone()
    member[1] = False                      # whole 16-byte groups overwritten
    member[1, V - 1] = True
    member[2] = True                       # whole groups skipped
    member[2, 9] = False
    allowed = _pack(member)
    want = logits.clone().masked_fill(~member.to(DEV), float("-inf"))
    x = logits.clone()
    assert ops.mask_logits_(x, allowed) is x
    torch.cuda.synchronize()
    assert _bits_equal(x, want)
    ones = torch.full_like(allowed, -1)
    y = logits.clone()
    ops.mask_logits_(y, ones)
    torch.cuda.synchronize()
    assert _bits_equal(y, logits)


# (row stride, first column, width): vector rows; vector rows with a
# V % 8 tail; rows whose stride breaks 16-byte alignment; a misaligned base
@pytest.mark.parametrize("ld,c0,V", [(1024, 8, 1000), (1000, 0, 997),
                                     (1003, 0, 1000), (1024, 1, 1000)])
def test_mask_logits_row_strides(ld, c0, V):
    g = torch.Generator().manual_seed(ld + c0)
    big = (torch.randn(B, ld, generator=g) * 3.0).to(torch.bfloat16).to(DEV)
    member = torch.rand(B, V, generator=g) < 0.5
    member[3] = False
    full = torch.ones(B, ld, dtype=torch.bool)
    full[:, c0:c0 + V] = member
    want = big.clone().masked_fill(~full.to(DEV), float("-inf"))
    view = big[:, c0:c0 + V]
    assert view.stride(0) == ld and not view.is_contiguous()
    ops.mask_logits_(view, _pack(member))
    torch.cuda.synchronize()
    assert _bits_equal(big, want)          # columns outside the view intact


# -------------------------------------------------------------------- engine
def _engine(graphs, seed=11):
    return LLMEngine(CONFIGS["tiny"], device="cuda", page_size=4,
                     num_pages=128, max_num_seqs=4, enable_graphs=graphs,
                     seed=seed)


def _run(eng, reqs):
    rids = [eng.add_request(p, sp) for p, sp in reqs]
    fins = {}
    for _ in range(400):
        eng.step()
        for r in rids:
            if r not in fins:
                f = eng.get_finished(r)
                if f:
                    fins[r] = f
        if len(fins) == len(rids):
            break
    assert len(fins) == len(rids)
    return [fins[r] for r in rids]


def _parse_bytes(ids):
    body = ids[:-1] if ids and ids[-1] == 2 else ids
    return json.loads(bytes(b - 4 for b in body if 4 <= b < 260).decode(
        "utf-8", errors="replace"))


def test_engine_json_graph_matches_eager():
    reqs = [([1, 5 + i, 9], SamplingParams(max_tokens=6 + 5 * i,
                                           json_mode=True))
            for i in range(3)]
    reqs.append(([1, 40, 41], SamplingParams(max_tokens=12, ignore_eos=True)))
    outs = {}
    for graphs in (False, True):
        eng = _engine(graphs)
        outs[graphs] = [f.output_ids for f in _run(eng, reqs)]
        m = eng.metrics
        assert m["decode_graph_steps"] + m["decode_eager_steps"] == \
            m["decode_steps"]
        if graphs:
            assert m["decode_eager_steps"] == 0
            assert m["decode_graph_steps"] > 0
            assert any(k[3] for k in eng._graphs), eng._graphs.keys()
        else:
            assert m["decode_graph_steps"] == 0 and not eng._graphs
    assert outs[False] == outs[True]
    for ids in outs[True][:3]:
        _parse_bytes(ids)
    assert len(outs[True][3]) == 12


def test_engine_json_sampled_in_graph():
    from agentfield_amd.engine.schemafsm import SchemaSpec
    eng = _engine(True)
    fins = _run(eng, [([1, 5 + i, 9], SamplingParams(
        max_tokens=8 + 4 * i, temperature=0.9, json_mode=True))
        for i in range(3)])
    for f in fins:
        _parse_bytes(f.output_ids)
    assert eng.metrics["decode_eager_steps"] == 0
    assert eng.metrics["decode_graph_steps"] > 0

    spec = SchemaSpec({"type": "object",
                       "properties": {"x": {"type": "integer"},
                                      "s": {"enum": ["a", "bb"]}},
                       "required": ["x"]})
    eng = _engine(True)
    fins = _run(eng, [([1, 30 + i, 9], SamplingParams(
        max_tokens=24, temperature=0.9, json_mode=True, json_schema=spec))
        for i in range(4)])
    for f in fins:
        data = _parse_bytes(f.output_ids)
        assert isinstance(data["x"], int) and set(data) <= {"x", "s"}
        if "s" in data:
            assert data["s"] in ("a", "bb")
    assert eng.metrics["decode_eager_steps"] == 0
    assert eng.metrics["decode_graph_steps"] > 0


def test_engine_logprobs_under_mask():
    """Greedy under a grammar: the chosen token is the best LEGAL token,
    so its logprob reaches the top-1 only if logprobs are taken over the
    masked logits (an illegal token outranks it otherwise)."""
    eng = _engine(True, seed=3)
    fin = _run(eng, [([1, 5, 9, 20], SamplingParams(
        max_tokens=10, json_mode=True, logprobs=3))])[0]
    assert fin.logprobs is not None
    assert len(fin.logprobs) == len(fin.output_ids)
    for e in fin.logprobs:
        # same tolerance as test_logprobs_in_graph_decode: the HIP sampler
        # and torch.topk break exact-bf16 ties differently
        assert e["logprob"] >= e["top"][0][1] - 1e-3
        assert e["logprob"] <= 0.0
    assert any(k[2] and k[3] for k in eng._graphs), eng._graphs.keys()
    assert eng.metrics["decode_eager_steps"] == 0
    _parse_bytes(fin.output_ids)
