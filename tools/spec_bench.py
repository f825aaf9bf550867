#!/usr/bin/env python3
"""Speculation acceptance benchmark: algorithmic speedup measured in
ENGINE STEPS (tokens emitted per decode step), which is hardware- and
timing-independent — the quantity a draft buys before kernel time
enters.  Random-init weights make a real draft useless, so the draft
case uses the TARGET as its own draft (the acceptance ceiling);
prompt-lookup is exercised with n-gram-rich prompts.

  python tools/spec_bench.py [--model tiny] [--gen 48] [--prompts 8]
"""
import argparse
import json
import random
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from agentfield_amd.engine import LLMEngine, SamplingParams
from agentfield_amd.models import CONFIGS


def run(cfg, prompts, gen, device, **spec_kw):
    kw = {}
    if device == "cpu":
        kw = {"dtype": torch.float32, "num_pages": 512, "page_size": 4,
              "enable_graphs": False}
    eng = LLMEngine(CONFIGS[cfg], device=device, max_num_seqs=8, seed=3,
                    **kw, **spec_kw)
    if spec_kw.get("draft_model") is None and "spec_draft" not in spec_kw \
            and not spec_kw.get("spec_lookup"):
        pass
    rids = [eng.add_request(p, SamplingParams(max_tokens=gen,
                                              ignore_eos=True))
            for p in prompts]
    outs = {}
    steps = 0
    while len(outs) < len(rids) and steps < 10000:
        eng.step()
        steps += 1
        for r in rids:
            if r not in outs:
                f = eng.get_finished(r)
                if f:
                    outs[r] = f.output_ids
    m = dict(eng.metrics)
    total = sum(len(o) for o in outs.values())
    return {
        "engine_steps": steps,
        "tokens": total,
        "tokens_per_step": round(total / max(1, steps), 2),
        "spec_steps": m["spec_steps"],
        "accept_rate": round(m["spec_accepted"] / m["spec_drafted"], 3)
        if m["spec_drafted"] else None,
        "outputs": [outs[r] for r in rids],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="tiny")
    ap.add_argument("--gen", type=int, default=48)
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--device", default=None,
                    help="default: cuda when a GPU is visible, else cpu")
    args = ap.parse_args()
    device = args.device or (
        "cuda" if torch.cuda.is_available() else "cpu")
    rng = random.Random(5)
    V = CONFIGS[args.model].vocab_size
    prompts = []
    for _ in range(args.prompts):
        pat = [rng.randrange(V) for _ in range(rng.randint(3, 5))]
        prompts.append((pat * 10)[:rng.randint(16, 28)])

    base = run(args.model, prompts, args.gen, device)
    lookup = run(args.model, prompts, args.gen, device,
                 spec_lookup=args.k)
    # acceptance CEILING: the target drafts for itself
    probe = LLMEngine(CONFIGS[args.model], device=device, seed=3,
                      **({"dtype": torch.float32, "num_pages": 512,
                          "page_size": 4, "enable_graphs": False}
                         if device == "cpu" else {}))
    ceiling = run(args.model, prompts, args.gen, device,
                  draft_model=probe.model, spec_draft_k=args.k)
    assert lookup["outputs"] == base["outputs"], "lookup not greedy-exact"
    assert ceiling["outputs"] == base["outputs"], "draft not greedy-exact"
    out = {
        "bench": "speculation_steps",
        "model": args.model, "device": device, "k": args.k,
        "baseline_tokens_per_step": base["tokens_per_step"],
        "lookup": {k: lookup[k] for k in
                   ("tokens_per_step", "accept_rate", "spec_steps")},
        "draft_ceiling": {k: ceiling[k] for k in
                          ("tokens_per_step", "accept_rate", "spec_steps")},
        "lookup_speedup": round(lookup["tokens_per_step"] /
                                base["tokens_per_step"], 2),
        "ceiling_speedup": round(ceiling["tokens_per_step"] /
                                 base["tokens_per_step"], 2),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
