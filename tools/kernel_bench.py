#!/usr/bin/env python3
"""Per-kernel microbenchmarks on MI355X: our HIP kernels vs roofline and
vs hipBLASLt (torch.matmul) where applicable.  Prints one JSON line per case.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from agentfield_amd import ops

DEV = "cuda"


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_gemm():
    for (M, N, K) in [(8192, 8192, 8192), (4096, 4096, 4096),
                      (8192, 14336 * 2, 4096), (16, 4096, 4096)]:
        a = torch.randn(M, K, dtype=torch.bfloat16, device=DEV)
        w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV)
        tf = 2.0 * M * N * K / 1e12
        t_ours = timeit(lambda: ops.gemm_bf16(a, w))
        t_blas = timeit(lambda: a @ w.t())
        row = {"op": "gemm_bf16", "MNK": [M, N, K],
               "ours_tflops": round(tf / t_ours, 1),
               "hipblaslt_tflops": round(tf / t_blas, 1)}
        if K % 32 == 0 and M >= 256:
            t_ring = timeit(lambda: ops.gemm_bf16_ring(a, w))
            row["ring_tflops"] = round(tf / t_ring, 1)
        if K % 64 == 0 and K >= 128 and M >= 256:
            t_q8 = timeit(lambda: ops.gemm_bf16_q8(a, w))
            row["q8_tflops"] = round(tf / t_q8, 1)
        if K % 128 == 0 and K >= 256 and M >= 256:
            from agentfield_amd.quant import quantize_mx
            a8, sa = quantize_mx(a.float().cpu())
            w8, sw = quantize_mx(w.float().cpu())
            a8, sa, w8, sw = (t.to(DEV) for t in (a8, sa, w8, sw))
            t_mx = timeit(lambda: ops.gemm_mxfp8(a8, sa, w8, sw))
            row["mxfp8_tflops"] = round(tf / t_mx, 1)
            # torch fp8 rowwise-scaled baseline when available
            try:
                af = a.float()
                wf = w.float()
                sa_r = af.abs().amax(1, keepdim=True) / 448.0
                sw_r = wf.abs().amax(1, keepdim=True) / 448.0
                a_f8 = (af / sa_r).to(torch.float8_e4m3fn)
                w_f8 = (wf / sw_r).to(torch.float8_e4m3fn)
                t_s = timeit(lambda: torch._scaled_mm(
                    a_f8, w_f8.t(), scale_a=sa_r, scale_b=sw_r.t(),
                    out_dtype=torch.bfloat16))
                row["scaled_mm_tflops"] = round(tf / t_s, 1)
            except Exception as e:
                row["scaled_mm_tflops"] = str(e)[:60]
        print(json.dumps(row))


def bench_skinny():
    for (M, N, K) in [(16, 6144, 4096), (16, 4096, 4096), (16, 28672, 4096),
                      (16, 4096, 14336), (64, 28672, 4096), (16, 128256, 4096),
                      (64, 4096, 14336), (64, 128256, 4096), (64, 6144, 4096),
                      (128, 6144, 4096), (128, 4096, 4096), (128, 28672, 4096),
                      (128, 4096, 14336)]:
        a = torch.randn(M, K, dtype=torch.bfloat16, device=DEV)
        w = torch.randn(N, K, dtype=torch.bfloat16, device=DEV)
        gb = N * K * 2 / 1e9
        t_ours = timeit(lambda: ops.linear_skinny(a, w), iters=30)
        t_blas = timeit(lambda: a @ w.t(), iters=30)
        print(json.dumps({"op": "gemm_skinny", "MNK": [M, N, K],
                          "ours_tbps": round(gb / t_ours / 1e3, 2),
                          "hipblaslt_tbps": round(gb / t_blas / 1e3, 2),
                          "ours_us": round(t_ours * 1e6, 1),
                          "blas_us": round(t_blas * 1e6, 1)}))
    bench_skinny_w8()


LLC_BYTES = 256 << 20   # MI355X Infinity Cache


def _rotation_us(fns, reps=7):
    """Median / min / max microseconds per call over `reps` passes through
    every callable of `fns` (one per distinct weight buffer)."""
    ts = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for fn in fns:
            fn()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1) * 1e3 / len(fns))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def bench_skinny_w8(ms=(16, 64, 128)):
    """bf16 vs MX-fp8 weight stream on the decode projections, same process,
    alternating.  Each path walks a rotation of distinct weight buffers
    larger than twice the last-level cache: a decode step never finds a
    layer's weights cached, a single reused matrix would be."""
    shapes = {"qkv": (6144, 4096), "o": (4096, 4096),
              "gate_up": (28672, 4096), "down": (4096, 14336)}
    for M in ms:
        for name, (N, K) in shapes.items():
            a = torch.randn(M, K, dtype=torch.bfloat16, device=DEV)
            b16, b8 = N * K * 2, N * K + N * K // 32
            n16 = 2 * LLC_BYTES // b16 + 2
            n8 = 2 * LLC_BYTES // b8 + 2
            w16 = [torch.randn(N, K, dtype=torch.bfloat16, device=DEV)
                   for _ in range(n16)]
            w8s = []
            for _ in range(n8):
                q = torch.randint(0, 256, (N, K), dtype=torch.uint8,
                                  device=DEV)
                q[(q & 0x7f) == 0x7f] = 0   # no NaN codes
                w8s.append((q, torch.randint(118, 124, (N, K // 32),
                                             dtype=torch.uint8, device=DEV)))
            f16 = [lambda w=w: ops.linear_skinny(a, w) for w in w16]
            f8 = [lambda wq=wq: ops.linear_skinny(a, w16[0], wq=wq)
                  for wq in w8s]
            _rotation_us(f16, reps=1), _rotation_us(f8, reps=1)   # warm up
            r16, r8 = [], []
            for _ in range(3):   # alternate the two paths
                r16.append(_rotation_us(f16))
                r8.append(_rotation_us(f8))
            m16 = sorted(r[0] for r in r16)[1]
            m8 = sorted(r[0] for r in r8)[1]
            lo16, hi16 = min(r[1] for r in r16), max(r[2] for r in r16)
            lo8, hi8 = min(r[1] for r in r8), max(r[2] for r in r8)
            row = {"op": "gemm_skinny_w8", "proj": name, "MNK": [M, N, K],
                   "bf16_us": round(m16, 1), "w8_us": round(m8, 1),
                   "bf16_tbps": round(b16 / m16 / 1e6, 2),
                   "w8_tbps": round(b8 / m8 / 1e6, 2),
                   "w8_over_bf16": round(m8 / m16, 3),
                   "bf16_spread_us": [round(lo16, 1), round(hi16, 1)],
                   "w8_spread_us": [round(lo8, 1), round(hi8, 1)],
                   "buffers": [n16, n8]}
            if M == 128 and name in ("qkv", "gate_up"):
                blas = [lambda w=w: a @ w.t() for w in w16]
                _rotation_us(blas, reps=1)
                row["blas_us"] = round(_rotation_us(blas)[0], 1)
            print(json.dumps(row), flush=True)
            del w16, w8s, f16, f8
            torch.cuda.empty_cache()


def bench_prefill(Hq=32, Hk=8, D=128, page=16):
    for (B, S) in [(16, 512), (4, 2048), (1, 8192)]:
        T = B * S
        q = torch.randn(T, Hq * D, dtype=torch.bfloat16, device=DEV)
        maxp = (S + page - 1) // page
        npages = 1 + B * maxp
        kc = torch.randn(npages, Hk, page, D, dtype=torch.bfloat16, device=DEV)
        vc = torch.randn_like(kc)
        bt = torch.arange(1, npages, dtype=torch.int32,
                          device=DEV).reshape(B, maxp)
        cu = torch.arange(0, T + 1, S, dtype=torch.int32, device=DEV)
        qstart = torch.zeros(B, dtype=torch.int32, device=DEV)
        lens = [S] * B
        # causal flops: 2 * (QK + PV) * 0.5 * S^2 * D * Hq per seq
        tf = 2.0 * 2 * 0.5 * S * S * D * Hq * B / 1e12
        t = timeit(lambda: ops.attn_prefill(q, kc, vc, bt, qstart, cu, lens))
        print(json.dumps({"op": "attn_prefill_paged", "B": B, "S": S,
                          "tflops": round(tf / t, 1), "ms": round(t * 1e3, 3)}))


def bench_decode(Hq=32, Hk=8, D=128, page=None):
    import itertools
    for (B, L, nsplit), page in itertools.product(
            [(16, 576, 4), (128, 576, 1), (64, 1024, 1), (256, 1024, 1)],
            (16, 32, 64)):
        npages = B * ((L + page - 1) // page) + 1
        q = torch.randn(B, Hq * D, dtype=torch.bfloat16, device=DEV)
        kc = torch.randn(npages, Hk, page, D, dtype=torch.bfloat16, device=DEV)
        vc = torch.randn_like(kc)
        maxp = (L + page - 1) // page
        bt = torch.arange(1, npages, dtype=torch.int32, device=DEV).reshape(B, maxp)
        lens = torch.full((B,), L, dtype=torch.int32, device=DEV)
        gb = 2.0 * B * L * Hk * D * 2 / 1e9  # K+V bytes read
        t = timeit(lambda: ops.attn_decode(q, kc, vc, bt, lens, nsplit=nsplit))
        print(json.dumps({"op": "attn_decode", "B": B, "L": L, "page": page,
                          "nsplit": nsplit, "gbps": round(gb / t, 1),
                          "us": round(t * 1e6, 1)}))


def bench_norm_rope(H=4096):
    for T in (16, 8192):
        x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV)
        w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
        res = torch.randn_like(x)
        gb = 4.0 * T * H * 2 / 1e9  # read x,res; write out,res
        t = timeit(lambda: ops.rmsnorm(x, w, 1e-5, residual=res))
        print(json.dumps({"op": "rmsnorm_fused", "T": T, "gbps": round(gb / t, 1),
                          "us": round(t * 1e6, 1)}))
        gu = torch.randn(T, 28672, dtype=torch.bfloat16, device=DEV)
        gb2 = (T * 28672 + T * 14336) * 2 / 1e9
        t2 = timeit(lambda: ops.silu_and_mul(gu))
        print(json.dumps({"op": "silu_mul", "T": T, "gbps": round(gb2 / t2, 1),
                          "us": round(t2 * 1e6, 1)}))
    x = torch.randn(65536, H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
    res = torch.randn_like(x)
    gb = 4.0 * 65536 * H * 2 / 1e9
    t = timeit(lambda: ops.rmsnorm(x, w, 1e-5, residual=res), iters=10)
    print(json.dumps({"op": "rmsnorm_fused", "T": 65536,
                      "gbps": round(gb / t, 1), "us": round(t * 1e6, 1)}))


def bench_sample(B=64, V=128256):
    logits = torch.randn(B, V, dtype=torch.bfloat16, device=DEV)
    st = ops.SamplerState(B, DEV)
    temps = torch.full((B,), 0.8, device=DEV)
    t = timeit(lambda: ops.sample(logits, temps, st))
    print(json.dumps({"op": "sample", "B": B, "V": V, "us": round(t * 1e6, 1)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    for name, fn in [("gemm", bench_gemm), ("skinny", bench_skinny),
                     ("prefill", bench_prefill),
                     ("decode", bench_decode), ("norm", bench_norm_rope),
                     ("sample", bench_sample)]:
        if args.only in (None, name):
            fn()
