"""The MX-fp4 weight-streaming skinny GEMM (csrc/gemm_skinny_w4.hip) and the
quant="mxfp4" decode path.  The kernel rebuilds the bf16 numbers of
dequantize_mx4(w4, sw) and runs gemm_skinny_kernel's arithmetic on them, so
every comparison with the bf16 kernel on that matrix is torch.equal.

K=64 has no pipelined step; K=320 with sk=2 gives Kc=192 (a split ends and
the next begins inside a 256-K W4 line); K=576 is two lines plus a 64-K tail.
M=17 crosses the M-tile edge, 49 is the first size with one X sub-tile per
step, 65 starts the second 64-row X block, 256 is MT=16.
"""
import functools

import pytest
import torch

import attn_cases as ac
from agentfield_amd import ops
from agentfield_amd.quant import dequantize_mx4, quantize_mx4

pytestmark = pytest.mark.gpu
DEV = "cuda"
REDUCED = [(m, n, k) for m in (1, 65) for n in (64, 192) for k in (64, 320)]


@functools.lru_cache(maxsize=None)
def _weights(N, K, raw=False):
    """(w4, sw, wd) on the device.  Quantised: magnitudes vary per row and
    per K-block (2^-8..2^8), so data under the wrong scale cannot cancel.
    raw: all 256 byte values, scale bytes in [100, 140], zero nibbles under
    non-trivial scales; pins nibble order, code table and +-0."""
    g = ac.gen(7000 + N + K + raw)
    if raw:
        w4 = torch.randint(0, 256, (N * K // 2,), generator=g).to(torch.uint8)
        w4[:256] = torch.randperm(256, generator=g).to(torch.uint8)
        w4 = w4.reshape(N, K // 2)[torch.randperm(N, generator=g)].contiguous()
        sw = torch.randint(100, 141, (N, K // 32), generator=g).to(torch.uint8)
        zero = (((w4 & 7) == 0) | ((w4 & 0x70) == 0)).reshape(N, -1, 16).any(-1)
        assert w4.unique().numel() == 256 and (sw[zero] != 127).any()
    else:
        e = torch.randint(-8, 9, (N, K // 32, 1), generator=g).float()
        w4, sw = quantize_mx4((torch.randn(N, K // 32, 32, generator=g) * 0.05
                               * torch.pow(2.0, e)).reshape(N, K))
    d = dequantize_mx4(w4, sw)
    assert torch.equal(d.bfloat16().float(), d)
    return w4.to(DEV), sw.to(DEV), d.bfloat16().to(DEV)


def _x(M, K, seed=0):
    return ac.randn_bf16(ac.gen(9000 + M + K + seed), M, K).to(DEV)


def _check_same(x, wts, **kw):
    """fp4 path == bf16 path on the dequantized matrix, for every sk: out,
    updated residual and ss_out."""
    w4, sw, wd = wts
    for sk in (1, 2, None):
        res = []
        for wq4 in ((w4, sw), None):
            k = {n: (v.clone() if n == "residual" else
                     torch.full_like(v, float("nan")) if n == "ss_out" else v)
                 for n, v in kw.items()}
            out = ops.linear_skinny(x, wd, wq4=wq4, sk=sk, **k)
            res.append((out, k.get("residual"), k.get("ss_out")))
        for a, b in zip(*res):
            if a is not None:
                assert not torch.isnan(a.float()).any()
                assert torch.equal(a, b), (sk, (a != b).sum().item())
    return res[0]


@pytest.mark.parametrize("raw,M", [(False, m) for m in (1, 17, 49, 65, 256)]
                         + [(True, 1), (True, 65)])
@pytest.mark.parametrize("K", [64, 320, 576])
@pytest.mark.parametrize("N", [64, 192])
def test_w4_exact_mode0(M, N, K, raw):
    out, _, _ = _check_same(_x(M, K), _weights(N, K, raw))
    assert out.shape == (M, N)


@pytest.mark.parametrize("mode,scaled", [(2, False), (0, True), (2, True)])
@pytest.mark.parametrize("M,N,K", REDUCED)
def test_w4_exact_mode2_and_scale(M, N, K, mode, scaled):
    kw = {}
    if scaled:
        ss = (torch.rand(M, 8, generator=ac.gen(9500 + M + K)) + 0.5) * K / 8
        kw["scale"] = (ss.to(DEV), 1e-5)
    out, _, _ = _check_same(_x(M, K, 2), _weights(N, K), mode=mode, **kw)
    assert out.shape == (M, N // 2 if mode == 2 else N)


@pytest.mark.parametrize("M,N,K", REDUCED)
def test_w4_exact_mode4(M, N, K):
    res = ac.randn_bf16(ac.gen(9900 + M + N), M, N).to(DEV)
    out, new_res, _ = _check_same(
        _x(M, K, 4), _weights(N, K), mode=4, residual=res,
        ss_out=torch.empty(M, 8, dtype=torch.float32, device=DEV))
    assert torch.equal(out, new_res) and not torch.equal(new_res, res)


def test_w4_vs_fp64():
    """Against an oracle that is not its sibling: fp64 x @ wd.T, budgeted by
    the fp32-math CPU counterpart."""
    M, N, K = 128, 192, 320
    x, (w4, sw, wd) = _x(M, K, 5), _weights(N, K)
    out = ops.linear_skinny(x, wd, wq4=(w4, sw))
    xc, wc = x.cpu(), wd.cpu()
    ac.budget_check(f"skinny-w4 {M}x{N}x{K}", out.cpu(), ac.skinny_cpu(xc, wc),
                    xc.to(ac.F64) @ wc.to(ac.F64).t())


@pytest.mark.parametrize("B", [3, 70])
def test_model_decode_step_w4_equals_bf16(B, monkeypatch):
    """One decode step of a folded, quantised tiny model: logits through the
    fp4 stream == logits with no_w8_decode.  B=3: 4 GEMMs per layer carry
    wq4; B=70: qkv / gate_up go to hipBLASLt, 2 per layer."""
    from agentfield_amd.models.llama import LlamaForCausalLM
    c = ac.step_case(B)
    model = LlamaForCausalLM(c.cfg, device=DEV)
    model.load_state_dict(c.model.state_dict())
    model._norms_folded = True
    model.quantize_weights("mxfp4")
    model.w4_min_elems = 0   # tiny's matrices are below the serving cut-off
    calls, real = [], ops.linear_skinny
    monkeypatch.setattr(ops, "linear_skinny", lambda *a, **kw: (
        calls.append(kw.get("wq4") is not None), real(*a, **kw))[1])
    logits = {}
    for on in (True, False):
        model.no_w8_decode = not on
        calls.clear()
        with torch.no_grad():
            logits[on] = model(c.ids.to(DEV), c.pos.to(DEV), c.kv(DEV),
                               c.metadata(DEV))
        assert sum(calls) == ((4 if B <= 64 else 2) * c.cfg.num_layers) * on
    assert not torch.isnan(logits[True].float()).any()
    assert torch.equal(logits[True], logits[False])


def test_engine_generate_w4_equals_bf16():
    from agentfield_amd.engine import LLMEngine, SamplingParams
    from agentfield_amd.models import CONFIGS
    prompts = [[1, 5, 9, 20, 7], [3, 7, 11], [2, 4, 6, 8]]
    outs = {}
    for on in (True, False):
        eng = LLMEngine(CONFIGS["tiny"], device="cuda", quant="mxfp4",
                        enable_graphs=True, page_size=4, num_pages=128,
                        max_num_seqs=4, seed=3)
        eng.model.no_w8_decode = not on
        eng.model.w4_min_elems = 0   # every projection through the fp4 kernel
        outs[on] = eng.generate(prompts, SamplingParams(max_tokens=8,
                                                        ignore_eos=True))
        assert eng.metrics["decode_graph_steps"] > 0
    assert all(len(o) == 8 for o in outs[True]) and outs[True] == outs[False]
