"""The MX-fp8 weight-streaming skinny GEMM (csrc/gemm_skinny_w8.hip) and the
quant="mxfp8" decode path built on it.

The kernel rebuilds in registers the very bf16 numbers that
dequantize_mx(w8, sw).bfloat16() holds and runs gemm_skinny_kernel's
arithmetic on them, so every comparison against the bf16 kernel on the
dequantized matrix is torch.equal: no tolerance anywhere but in the one
independent fp64 check.

Shapes: K=64 has no pipelined step; K=320 with sk=2 splits unevenly
(Kc=192: 192+128, odd step count); N=192 exercises the nblk offsets; M=17, 65,
256 hit the M-tile edge, the second X stage block and the MT=16 arm.
"""
import copy
import functools

import pytest
import torch

import attn_cases as ac
from agentfield_amd import ops
from agentfield_amd.quant import dequantize_mx, quantize_mx

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
MS = [1, 17, 64, 65, 128, 256]
NS = [64, 192]
KS = [64, 128, 320]
SKS = [1, 2, None]
# reduced grid for the fused epilogues: both N, the unpipelined and the
# uneven-split K, the M-tile edge / second stage block / MT=16 arms
REDUCED = [(m, n, k) for m in (1, 17, 65, 256) for n in NS for k in (64, 320)]


@functools.lru_cache(maxsize=None)
def _quantised(N, K):
    """(w8, sw, wd) on the device.  Magnitudes vary per row AND per K-block
    (2^-8..2^8), so data paired with another block's or row's scale cannot
    cancel."""
    g = ac.gen(7000 + N + K)
    e = torch.randint(-8, 9, (N, K // 32, 1), generator=g).float()
    w = (torch.randn(N, K // 32, 32, generator=g) * 0.05
         * torch.pow(2.0, e)).reshape(N, K)
    w8, sw = quantize_mx(w)
    assert sw.unique().numel() > 8
    return _on_device(w8, sw)


@functools.lru_cache(maxsize=None)
def _raw_codes(N, K):
    """(w8, sw, wd) from raw bytes: all 254 non-NaN e4m3 codes present
    (0x00 and 0x80 included, several times, under non-trivial scales), scale
    bytes uniform in [100, 140]."""
    g = ac.gen(8000 + N + K)
    codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f],
                         dtype=torch.uint8)
    assert codes.numel() == 254
    flat = codes[torch.randint(0, 254, (N * K,), generator=g)]
    flat[:254] = codes[torch.randperm(254, generator=g)]
    zeros = torch.randperm(N * K - 254, generator=g)[:64] + 254
    flat[zeros[:32]] = 0x00
    flat[zeros[32:]] = 0x80
    w8 = flat.reshape(N, K)[torch.randperm(N, generator=g)].contiguous()
    assert w8.unique().numel() == 254
    sw = torch.randint(100, 141, (N, K // 32), generator=g).to(torch.uint8)
    zero_blocks = (w8.reshape(N, K // 32, 32) & 0x7f).eq(0).any(-1)
    assert (sw[zero_blocks] != 127).any(), "zeros need non-trivial scales"
    return _on_device(w8, sw)


def _on_device(w8, sw):
    d = dequantize_mx(w8, sw)
    wd = d.bfloat16()
    assert torch.equal(wd.float(), d), "the MX grid must be exact in bf16"
    return w8.to(DEV), sw.to(DEV), wd.to(DEV)


def _x(M, K, seed=0):
    return ac.randn_bf16(ac.gen(9000 + M + K + seed), M, K).to(DEV)


def _ss8(M, K):
    g = ac.gen(9500 + M + K)
    return ((torch.rand(M, 8, generator=g) + 0.5) * K / 8).to(DEV)


def _both(x, wts, **kw):
    """(w8 path, bf16 path on the dequantized matrix); a residual is cloned
    per path and returned updated."""
    w8, sw, wd = wts
    outs = []
    for wq in ((w8, sw), None):
        k = dict(kw)
        if "residual" in k:
            k["residual"] = k["residual"].clone()
        if "ss_out" in k:
            k["ss_out"] = torch.full_like(k["ss_out"], float("nan"))
        out = ops.linear_skinny(x, wd, wq=wq, **k)
        outs.append((out, k.get("residual"), k.get("ss_out")))
    torch.cuda.synchronize()
    return outs


def _assert_same(tag, got, want):
    for name, a, b in zip(("out", "residual", "ss_out"), got, want):
        if a is None:
            assert b is None
            continue
        assert not torch.isnan(a.float()).any(), f"{tag}: {name} has NaN"
        assert torch.equal(a, b), (
            f"{tag}: {name} differs in {(a != b).sum().item()} of "
            f"{a.numel()} elements, max |d| "
            f"{(a.float() - b.float()).abs().max().item():.3e}")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_w8_exact_mode0(M, N, K):
    x, wts = _x(M, K), _quantised(N, K)
    for sk in SKS:
        got, want = _both(x, wts, sk=sk)
        assert got[0].shape == (M, N)
        _assert_same(f"mode0 {M}x{N}x{K} sk={sk}", got, want)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_w8_exact_raw_codes(M, N, K):
    """Pins the byte -> value table and +-0 under any scale, independently
    of quantize_mx."""
    x, wts = _x(M, K, seed=1), _raw_codes(N, K)
    for sk in SKS:
        got, want = _both(x, wts, sk=sk)
        _assert_same(f"raw {M}x{N}x{K} sk={sk}", got, want)


@pytest.mark.parametrize("M", [16, 32, 33, 48, 49])
def test_w8_exact_m_tile_arms(M):
    """The kernel stages only the X rows its M tiles use and, up to three
    tiles, two 64-K sub-tiles per step: both sides of each boundary, on the
    uneven split (a one-sub-tile last step) and the unpipelined K."""
    for K in (64, 320):
        x, wts = _x(M, K, seed=6), _raw_codes(192, K)
        for sk in SKS:
            got, want = _both(x, wts, sk=sk)
            _assert_same(f"arms {M}x192x{K} sk={sk}", got, want)


@pytest.mark.parametrize("M,N,K", REDUCED)
def test_w8_exact_mode2(M, N, K):
    x, wts = _x(M, K, seed=2), _quantised(N, K)
    for sk in SKS:
        got, want = _both(x, wts, sk=sk, mode=2)
        assert got[0].shape == (M, N // 2)
        _assert_same(f"mode2 {M}x{N}x{K} sk={sk}", got, want)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("M,N,K", REDUCED)
def test_w8_exact_with_scale(M, N, K, mode):
    x, wts = _x(M, K, seed=3), _quantised(N, K)
    ss = _ss8(M, K)
    for sk in SKS:
        got, want = _both(x, wts, sk=sk, mode=mode, scale=(ss, EPS))
        _assert_same(f"scale mode{mode} {M}x{N}x{K} sk={sk}", got, want)


@pytest.mark.parametrize("M,N,K", REDUCED)
def test_w8_exact_mode4(M, N, K):
    x, wts = _x(M, K, seed=4), _quantised(N, K)
    res = ac.randn_bf16(ac.gen(9900 + M + N), M, N).to(DEV)
    ss_out = torch.empty(M, 8, dtype=torch.float32, device=DEV)
    for sk in SKS:
        got, want = _both(x, wts, sk=sk, mode=4, residual=res, ss_out=ss_out)
        assert torch.equal(got[0], got[1]), "residual must equal the output"
        assert not torch.equal(got[1], res), "residual was not updated"
        _assert_same(f"mode4 {M}x{N}x{K} sk={sk}", got, want)


def test_w8_vs_fp64():
    """The new kernel against an oracle that is not its sibling: fp64
    x @ wd.T, budgeted by the fp32-math CPU counterpart."""
    M, N, K = 128, 192, 320
    x, (w8, sw, wd) = _x(M, K, seed=5), _quantised(N, K)
    out = ops.linear_skinny(x, wd, wq=(w8, sw))
    torch.cuda.synchronize()
    xc, wc = x.cpu(), wd.cpu()
    W = ac.skinny_cpu(xc, wc)
    T = xc.to(ac.F64) @ wc.to(ac.F64).t()
    ac.budget_check(f"skinny-w8 {M}x{N}x{K}", out.cpu(), W, T)


def test_w8_rejects_bad_operands_on_device():
    x, (w8, sw, wd) = _x(4, 64), _quantised(64, 64)
    with pytest.raises(ValueError):
        ops.linear_skinny(x, wd, wq=(w8.cpu(), sw))
    with pytest.raises(ValueError):
        ops.linear_skinny(x, wd, wq=(w8, sw.to(torch.int32)))


@pytest.mark.parametrize("B", [3, 70])
def test_model_decode_step_w8_equals_bf16(B, monkeypatch):
    """One decode step of a folded, quantised tiny model over a prefilled
    cache: logits through the fp8 stream == logits with no_w8_decode.
    B=3 takes the skinny branch (4 GEMMs per layer carry wq), B=70 the
    hipBLASLt branch for qkv / gate_up (2 per layer)."""
    from agentfield_amd.models.llama import LlamaForCausalLM
    c = ac.step_case(B)
    model = LlamaForCausalLM(c.cfg, device=DEV)
    model.load_state_dict(c.model.state_dict())
    model._norms_folded = True
    before = copy.deepcopy(model.state_dict())
    model.quantize_weights("mxfp8")
    model.w8_min_elems = 0   # tiny's matrices are below the serving cut-off
    assert not torch.equal(model.layers[0].attn.o, before["layers.0.attn.o"])
    assert model.layers[0].attn.o_q8.is_cuda

    calls = []
    real = ops.linear_skinny

    def counting(*a, **kw):
        calls.append(kw.get("wq") is not None)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "linear_skinny", counting)
    ids, pos, md = c.ids.to(DEV), c.pos.to(DEV), c.metadata(DEV)
    logits = {}
    for w8_on in (True, False):
        model.no_w8_decode = not w8_on
        calls.clear()
        assert model._can_fuse_decode(B)
        with torch.no_grad():
            logits[w8_on] = model(ids, pos, c.kv(DEV), md)
        torch.cuda.synchronize()
        # (the lm_head may add one skinny call of its own, never with wq)
        per_layer = 4 if B <= 64 else 2
        assert len(calls) >= per_layer * c.cfg.num_layers
        assert sum(calls) == (per_layer * c.cfg.num_layers if w8_on else 0)
    assert not torch.isnan(logits[True].float()).any()
    assert torch.equal(logits[True], logits[False])


def test_model_decode_w8_size_cutoff(monkeypatch):
    """Default dispatch: at M <= 64 a matrix below w8_min_elems keeps its
    bf16 stream; above 64 rows o and down stream as fp8 whatever their size."""
    from agentfield_amd.models.llama import LlamaForCausalLM
    seen = []
    real = ops.linear_skinny

    def recording(x, w, *a, **kw):
        seen.append((x.shape[0], w, kw.get("wq") is not None))
        return real(x, w, *a, **kw)

    monkeypatch.setattr(ops, "linear_skinny", recording)
    for B in (3, 70):
        c = ac.step_case(B)
        model = LlamaForCausalLM(c.cfg, device=DEV)
        model.load_state_dict(c.model.state_dict())
        model._norms_folded = True
        model.quantize_weights("mxfp8")
        assert model.w8_min_elems == 1 << 25
        model.w8_min_elems = model.layers[0].mlp.down.numel() + 1
        seen.clear()
        with torch.no_grad():
            model(c.ids.to(DEV), c.pos.to(DEV), c.kv(DEV), c.metadata(DEV))
        torch.cuda.synchronize()
        layer_calls = [s for s in seen if s[1] is not model.lm_head]
        assert len(layer_calls) == (4 if B <= 64 else 2) * c.cfg.num_layers
        for M, w, used in layer_calls:
            assert used == (M > 64 or w.numel() >= model.w8_min_elems)
        assert any(u for *_, u in layer_calls), "no call took the fp8 path"


def test_engine_generate_w8_equals_bf16():
    from agentfield_amd.engine import LLMEngine, SamplingParams
    from agentfield_amd.models import CONFIGS
    prompts = [[1, 5, 9, 20, 7], [3, 7, 11], [2, 4, 6, 8]]
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    outs = {}
    for w8_on in (True, False):
        eng = LLMEngine(CONFIGS["tiny"], device="cuda", quant="mxfp8",
                        enable_graphs=True, page_size=4, num_pages=128,
                        max_num_seqs=4, seed=3)
        assert eng.model.quant == "mxfp8" and eng.model._norms_folded
        eng.model.no_w8_decode = not w8_on
        eng.model.w8_min_elems = 0   # every projection through the fp8 kernel
        outs[w8_on] = eng.generate(prompts, sp)
        assert eng.metrics["decode_graph_steps"] > 0
        del eng
        torch.cuda.empty_cache()
    assert all(len(o) == 8 for o in outs[True])
    assert outs[True] == outs[False]
