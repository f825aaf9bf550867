"""MXFP8 quantization (OCP e4m3 + E8M0 per-32-block scales) for the
CDNA4 scaled MFMA path (mfma_scale_*_f8f6f4 — hardware-fused
dequant+matmul at 2x the bf16 rate), and MXFP4 (OCP e2m1, same scales,
two codes per byte) for the fp4 weight-streaming decode GEMM.

Weight-only or W8A8 quantized serving is opt-in; the bf16 path stays
the default (BASELINE dtype).
"""
from __future__ import annotations

import torch

BLOCK = 32          # MX scale granularity along K
FP8_MAX = 448.0     # e4m3fn max magnitude


def quantize_mx(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[R, K] float -> (e4m3 bytes [R, K] u8, E8M0 scales [R, K/32] u8).

    Per-block power-of-two scale: e = ceil(log2(absmax / FP8_MAX)), value
    stored as x / 2^e in e4m3, scale byte = e + 127 (E8M0 bias).  Exact
    powers of two round-trip losslessly; absmax maps inside fp8 range.
    """
    R, K = x.shape
    assert K % BLOCK == 0, "K must be a multiple of the MX block (32)"
    xf = x.float().reshape(R, K // BLOCK, BLOCK)
    amax = xf.abs().amax(dim=-1).clamp_min(1e-30)
    e = torch.ceil(torch.log2(amax / FP8_MAX)).clamp(-127, 127)
    scale = torch.pow(2.0, e)
    q = (xf / scale.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX)
    q8 = q.to(torch.float8_e4m3fn).view(torch.uint8).reshape(R, K)
    s8 = (e + 127).to(torch.uint8)
    return q8, s8


def dequantize_mx(q8: torch.Tensor, s8: torch.Tensor) -> torch.Tensor:
    """Inverse of quantize_mx (fp32)."""
    R, K = q8.shape
    v = q8.view(torch.float8_e4m3fn).float().reshape(R, K // BLOCK, BLOCK)
    e = s8.float() - 127.0
    return (v * torch.pow(2.0, e).unsqueeze(-1)).reshape(R, K)


# OCP e2m1: code = sign << 3 | exponent << 1 | mantissa
FP4_MAX = 6.0
FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mx4(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[R, K] float -> (e2m1 codes packed [R, K/2] u8, E8M0 scales
    [R, K/32] u8).

    Per-block power-of-two scale: e = ceil(log2(absmax / 6)), scale byte =
    e + 127 kept in 1..254.  x / 2^e is clamped to +-6 and rounded to the
    nearest e2m1 value, ties to the even code.  Element k sits in byte
    k >> 1, even k in the low nibble.  A value that rounds to zero gets
    code 0, never 8 (-0), so an all-zero block is all-zero bytes.
    """
    R, K = x.shape
    assert K % BLOCK == 0, "K must be a multiple of the MX block (32)"
    xf = x.float().reshape(R, K // BLOCK, BLOCK)
    amax = xf.abs().amax(dim=-1).clamp_min(1e-30)
    e = torch.ceil(torch.log2(amax / FP4_MAX)).clamp(-126, 127)
    a = (xf.abs() / torch.pow(2.0, e).unsqueeze(-1)).clamp(max=FP4_MAX)
    # midpoints between neighbouring values; a tie goes to the even code
    mag = ((a > 0.25).int() + (a >= 0.75).int() + (a > 1.25).int()
           + (a >= 1.75).int() + (a > 2.5).int() + (a >= 3.5).int()
           + (a > 5.0).int())
    code = (mag | (((xf < 0) & (mag > 0)).int() << 3)).reshape(R, K // 2, 2)
    q4 = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    s8 = (e + 127).to(torch.uint8)
    return q4, s8


def dequantize_mx4(q4: torch.Tensor, s8: torch.Tensor) -> torch.Tensor:
    """Inverse of quantize_mx4 (fp32), by table lookup; code 8 is -0."""
    R, K2 = q4.shape
    K = 2 * K2
    table = torch.tensor(FP4_VALUES + tuple(-v for v in FP4_VALUES),
                         dtype=torch.float32, device=q4.device)
    codes = torch.stack((q4 & 0xf, q4 >> 4), dim=-1).reshape(R, K)
    v = table[codes.long()].reshape(R, K // BLOCK, BLOCK)
    e = s8.float() - 127.0
    return (v * torch.pow(2.0, e).unsqueeze(-1)).reshape(R, K)
