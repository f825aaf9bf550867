"""Packed grammar token masks on the CPU: the pack/unpack helpers, the
reference paths of ops.sample(allowed=) and ops.mask_logits_, the
grammar's cached bit rows, and a mixed constrained/unconstrained batch
through the CPU engine."""
import json
import random

import pytest
import torch

from agentfield_amd import ops
from agentfield_amd.engine import LLMEngine, SamplingParams
from agentfield_amd.engine.jsonfsm import JsonFSM
from agentfield_amd.engine.token_grammar import TokenJsonGrammar
from agentfield_amd.models import CONFIGS
from test_token_grammar import FakeBPE

VS = (1, 31, 32, 33, 1000, 128256)


def _bit(bits: torch.Tensor, v: int) -> int:
    return (int(bits[v >> 5]) >> (v & 31)) & 1


@pytest.mark.parametrize("V", VS)
def test_pack_unpack_round_trip(V):
    W = (V + 31) // 32
    g = torch.Generator().manual_seed(V)
    member = torch.rand(V, generator=g) < 0.5
    ids = member.nonzero().flatten().tolist()
    sparse = sorted({0, V - 1, V // 2})
    cases = [(member, member), (ids, member),
             (torch.tensor(ids, dtype=torch.int64), member),
             ([], torch.zeros(V, dtype=torch.bool)),
             (torch.zeros(V, dtype=torch.bool), torch.zeros(V, dtype=torch.bool)),
             (list(range(V)), torch.ones(V, dtype=torch.bool)),
             (torch.ones(V, dtype=torch.bool), torch.ones(V, dtype=torch.bool)),
             (sparse, torch.zeros(V, dtype=torch.bool).index_fill_(
                 0, torch.tensor(sparse), True))]
    for src, want in cases:
        bits = ops.pack_token_mask(src, V)
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (W,)
        assert torch.equal(ops.unpack_token_mask(bits, V), want)
        # the format itself, not just the inverse: LSB-first bit v & 31 of
        # word v >> 5
        for v in {0, V - 1, V // 2, min(V - 1, 31), min(V - 1, 32)}:
            assert _bit(bits, v) == int(want[v])
        # tail bits of the last word are zero
        tail = W * 32 - V
        if tail:
            assert (int(bits[-1]) & 0xFFFFFFFF) >> (32 - tail) == 0
    # a full set is all ones up to the tail
    full = ops.pack_token_mask(list(range(V)), V)
    assert all(int(w) == -1 for w in full[:V // 32])


def test_pack_rejects_out_of_range_ids():
    with pytest.raises(ValueError):
        ops.pack_token_mask([0, 33], 33)
    with pytest.raises(ValueError):
        ops.pack_token_mask([-1], 33)


@pytest.mark.parametrize("V", (33, 1000))
def test_masked_greedy_cpu(V):
    g = torch.Generator().manual_seed(1)
    B = 4
    logits = torch.randn(B, V, generator=g)
    member = torch.rand(B, V, generator=g) < 0.5
    member[1] = False
    member[1, V - 1] = True                      # a single legal token
    member[0, logits[0].argmax()] = False        # global argmax disallowed
    member[3] = False                            # empty row -> token 0
    allowed = torch.stack([ops.pack_token_mask(m, V) for m in member])
    st = ops.SamplerState(B, "cpu")
    temps = torch.zeros(B)
    got = ops.sample(logits, temps, st, allowed=allowed)
    want = logits.masked_fill(~member, float("-inf")).argmax(-1).int()
    assert torch.equal(got, want)
    assert int(got[1]) == V - 1 and int(got[3]) == 0
    assert int(got[0]) != int(logits[0].argmax())
    ones = torch.full_like(allowed, -1)
    assert torch.equal(ops.sample(logits, temps, st, allowed=ones),
                       ops.sample(logits, temps, st))
    out = torch.zeros(B, dtype=torch.int32)
    ops.sample(logits, temps, st, out=out, allowed=allowed)
    assert torch.equal(out, want)


def test_mask_logits_cpu():
    V, B = 1000, 3
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(B, V, generator=g).to(torch.bfloat16)
    member = torch.rand(B, V, generator=g) < 0.3
    allowed = torch.stack([ops.pack_token_mask(m, V) for m in member])
    want = logits.clone().masked_fill(~member, float("-inf"))
    ret = ops.mask_logits_(logits, allowed)
    assert ret is logits
    assert torch.equal(logits.view(torch.int16), want.view(torch.int16))
    keep = logits.clone()
    ops.mask_logits_(logits, torch.full_like(allowed, -1))
    assert torch.equal(logits.view(torch.int16), keep.view(torch.int16))


def test_allowed_token_bits_match_ids_along_walk():
    tok = FakeBPE()
    g = TokenJsonGrammar(tok.vocab, eos_id=2)
    V = len(tok.vocab)

    def walk():
        rng = random.Random(5)
        steps = 0
        for _ in range(12):
            f = JsonFSM()
            budget = rng.choice([6, 12, 24])
            while budget > 0:
                ids = g.allowed_token_ids(f, budget)
                bits = g.allowed_token_bits(f, budget)
                assert torch.equal(bits, ops.pack_token_mask(ids, V))
                # a wider logits row (padded LM head) only adds zero words
                wide = g.allowed_token_bits(f, budget, V + 40)
                assert torch.equal(wide, ops.pack_token_mask(ids, V + 40))
                steps += 1
                t = rng.choice(ids)
                if t == 2:
                    break
                g.advance_token(f, t)
                budget -= 1
        return steps

    assert walk() > 50
    n_bits, n_ids = len(g._bits_cache), len(g._mask_cache)
    walk()
    assert len(g._bits_cache) == n_bits, "bits cache grew on a repeat walk"
    assert len(g._mask_cache) == n_ids
    # a hit hands back the cached row itself: the caller pays one row copy
    f = JsonFSM()
    assert g.allowed_token_bits(f, 24) is g.allowed_token_bits(f, 24)


def _engine():
    return LLMEngine(CONFIGS["tiny"], device="cpu", dtype=torch.float32,
                     page_size=4, num_pages=128, max_num_seqs=4,
                     enable_graphs=False, seed=6)


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


def test_byte_grammar_rows_cached_exactly():
    """The byte tokenizer's mask rows are memoized by PDA signature; a
    cached row must be the row the PDA computes at that state and budget
    (the budget class in the signature must not merge distinct masks)."""
    from agentfield_amd.engine.sequence import Sequence
    eng = _engine()
    V = eng.cfg.vocab_size
    rng = random.Random(9)
    checked = 0
    for trial in range(40):
        max_tokens = rng.choice([4, 9, 14, 30, 200])
        seq = Sequence(trial, [1], SamplingParams(max_tokens=max_tokens,
                                                  json_mode=True))
        fsm = JsonFSM()
        while len(seq.output_ids) < max_tokens:
            remaining = max_tokens - len(seq.output_ids)
            ids = fsm.allowed_token_ids(remaining)
            want = ops.pack_token_mask(ids, V)
            assert torch.equal(eng._json_allowed(seq), want), \
                (trial, seq.output_ids, remaining)
            checked += 1
            t = rng.choice(ids)
            if t == 2:
                break
            fsm.advance(t - 4)
            seq.output_ids.append(t)
    assert checked > 200
    assert 0 < len(eng._byte_bits) < checked  # rows were shared


def test_cpu_engine_mixed_constrained_batch():
    from agentfield_amd.sdk.ai import ByteTokenizer
    free = ([1, 40, 41, 42], SamplingParams(max_tokens=12, ignore_eos=True))
    alone = _run(_engine(), [free])[0].output_ids
    eng = _engine()
    fins = _run(eng, [
        ([1, 5, 9], SamplingParams(max_tokens=10, json_mode=True)),
        free,
        ([1, 7, 9], SamplingParams(max_tokens=16, json_mode=True)),
    ])
    # the grammar rows of its neighbours leave the unconstrained row alone
    assert fins[1].output_ids == alone
    tok = ByteTokenizer()
    for f in (fins[0], fins[2]):
        json.loads(tok.decode(f.output_ids).strip())
    m = eng.metrics
    assert m["decode_graph_steps"] == 0
    assert m["decode_eager_steps"] == m["decode_steps"] > 0
    assert not hasattr(eng, "_json_mask")
