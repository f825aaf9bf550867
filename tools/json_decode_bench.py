#!/usr/bin/env python3
"""Decode-step time of grammar-constrained (json_mode) batches against
unconstrained ones, at serving batch size.

Two cases on one engine configuration (random weights, byte tokenizer,
greedy rows so a run is reproducible):

  json   every row is json_mode
  plain  no constrained row (the existing captured decode step)

All rows stay alive for the whole run (ignore_eos, large max_tokens), so
every timed step decodes the full batch; the KV length grows by one per
step from --kv-len and the range is reported.  A step is timed with the
host clock around engine.step(), which ends in a stream synchronise.
Only full-batch decode steps are counted.  The timed steps are split
into --repeats windows and the spread of the window means is reported;
cases alternate window by window so drift hits both alike.

The tool uses only the engine's public surface, so the same file run
from a checkout of an older commit measures that commit (its json_mode
path decodes eagerly with a dense mask): that is how the "before" figure
in BENCHMARKS.md was taken.  Where the engine has them, the
graph/eager step counters and the host time spent producing the packed
mask rows are reported too.

  python tools/json_decode_bench.py [--model debug-1b] [--batch 128]
      [--kv-len 256] [--steps 32] [--repeats 6] [--warmup 16]
      [--vocab-size V] [--label COMMIT]
"""
import argparse
import dataclasses
import json
import random
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from agentfield_amd.engine import LLMEngine, SamplingParams
from agentfield_amd.models import CONFIGS


class Case:
    """One engine with a full batch in steady decode."""

    def __init__(self, name, cfg, args, device):
        self.name = name
        B, L = args.batch, args.kv_len
        total = args.warmup + args.steps * args.repeats + 8
        page = 64 if device == "cuda" else 4
        pages = B * ((L + total) // page + 2) + 16
        kw = {} if device == "cuda" else {"dtype": torch.float32}
        self.eng = LLMEngine(cfg, device=device, page_size=page,
                             num_pages=pages, max_num_seqs=B,
                             enable_graphs=device == "cuda", seed=3, **kw)
        self.fill_s = 0.0
        if hasattr(self.eng, "_fill_allow_rows"):  # host mask production
            inner = self.eng._fill_allow_rows

            def timed(rows, seqs):
                t0 = time.perf_counter()
                inner(rows, seqs)
                self.fill_s += time.perf_counter() - t0
            self.eng._fill_allow_rows = timed
        rng = random.Random(11)
        sp = SamplingParams(max_tokens=total + 8, ignore_eos=True,
                            json_mode=name == "json")
        for _ in range(B):
            prompt = [1] + [4 + rng.randrange(256) for _ in range(L - 1)]
            assert self.eng.add_request(prompt, sp) is not None
        self.B = B
        self.step_ms = []
        # prefill everything, then warm up on full-batch decode steps (the
        # first of them captures the graph where the engine uses one)
        full = tries = 0
        while full < args.warmup:
            before = self.eng.metrics["decode_steps"]
            ev = self.eng.step()
            if self.eng.metrics["decode_steps"] == before + 1 and \
                    len(ev) == B:
                full += 1
            tries += 1
            assert tries < 100 * (B + args.warmup), "never reached decode"
        self.fill_s = 0.0
        self.kv0 = L + self.eng.metrics["decode_steps"]

    def run(self, n):
        out = []
        for _ in range(n):
            before = self.eng.metrics["decode_steps"]
            t0 = time.perf_counter()
            ev = self.eng.step()
            dt = (time.perf_counter() - t0) * 1e3
            assert self.eng.metrics["decode_steps"] == before + 1 and \
                len(ev) == self.B, "batch fell out of steady decode"
            out.append(dt)
        self.step_ms.append(out)

    def report(self):
        wins = [statistics.fmean(w) for w in self.step_ms]
        flat = [x for w in self.step_ms for x in w]
        m = self.eng.metrics
        return {
            "step_ms_mean": round(statistics.fmean(wins), 3),
            "step_ms_median": round(statistics.median(flat), 3),
            "window_ms_min": round(min(wins), 3),
            "window_ms_max": round(max(wins), 3),
            "window_ms_stdev": round(statistics.stdev(wins), 3)
            if len(wins) > 1 else None,
            "timed_steps": len(flat),
            "kv_len": [self.kv0, self.kv0 + len(flat)],
            "graph_steps": m.get("decode_graph_steps"),
            "eager_steps": m.get("decode_eager_steps"),
            "mask_rows_host_ms_per_step":
                round(self.fill_s * 1e3 / len(flat), 3)
                if hasattr(self.eng, "_mask_words") else None,
        }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="debug-1b")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--kv-len", type=int, default=256)
    ap.add_argument("--steps", type=int, default=32,
                    help="decode steps per timing window")
    ap.add_argument("--repeats", type=int, default=6,
                    help="timing windows per case")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--vocab-size", type=int, default=0,
                    help="override the model's vocabulary size")
    ap.add_argument("--cases", default="json,plain")
    ap.add_argument("--label", default="",
                    help="commit the numbers belong to (reported as is)")
    ap.add_argument("--device", default="cuda",
                    help="cpu only rehearses the script; it times nothing "
                         "worth reporting")
    args = ap.parse_args()
    if args.device == "cuda" and not torch.cuda.is_available():
        sys.exit("json_decode_bench: no GPU visible (a CPU run measures "
                 "nothing; --device cpu only rehearses the script)")
    cfg = CONFIGS[args.model]
    if args.vocab_size:
        cfg = dataclasses.replace(cfg, vocab_size=args.vocab_size)
    cases = [Case(n, cfg, args, args.device) for n in args.cases.split(",")]
    for _ in range(args.repeats):
        for c in cases:
            c.run(args.steps)
    out = {"bench": "json_decode_step", "label": args.label,
           "model": args.model, "vocab_size": cfg.vocab_size,
           "batch": args.batch, "device": args.device,
           "steps_per_window": args.steps, "windows": args.repeats}
    out.update({c.name: c.report() for c in cases})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
