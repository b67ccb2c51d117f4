#!/usr/bin/env python
"""Times of the prior stage with exact lengths (DESIGN.md "Exact lengths", profiles/prior_exact_times.txt).

The seeded full model of tests/_flamed_common.build_flamed (bf16 decoder-side GEMMs, the package default), the
encoder output computed once, then per batch the three stages behind it -- PVA flow, length regulator, prior decode --
between device events (the regulator's host read of max(tgt_len) is inside):

  dense   PVA.sample + PriorHIP.decode              the padded batch (flamed_pva_flow, flamed_lr_lengths, flamed_prior_decode)
  exact   PVA.sample(exact=True) + decode(prompt_lens)   flamed_pva_flow_exact, flamed_lr_lengths_exact, flamed_prior_decode_lens
  alone   the utterances one after another, each a dense batch of one over its own phonemes and its own prompt
          (a timing: every batch of one draws its own noise, not the batch's slice, so its frame counts differ)

Batches: "a" = 4 utterances of 285 / 200 / 120 / 60 phonemes, nfe 64, prompts of 150 / 100 / 75 / 40 codes; "fixture" =
the two lines of tests/golden/flamed_sample.npz (12 / 9 phonemes, nfe 4), prompts of 20 / 13 codes.  Every figure is the
median (min .. max) of --reps calls after --warmup calls; every call re-seeds the CPU RNG, so all calls of one kind do
the same work.  "spread" is the largest (max - min) / median over the figures of a run: what one run calls noise.

--dense-only times the dense calls alone (all a library without the exact entry points can do: FLAMED_HIP_LIB pointing
at a build of the parent commit, alternated with this build, shows whether the dense path moved).  --dump FILE writes
the dense outputs of a seeded call (PVA states, tgt_len, prior_embs, logits) of both batches to an .npz; --compare FILE
compares this library's against such a file bitwise.  --persist prints how many of the exact flows ran as the
persistent launch.  One JSON line per figure on stdout."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "flamed-tts_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PAD = 1024


def timed(fn, reps, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": reps}


def batches():
    from _common import golden, t32
    g = torch.Generator().manual_seed(2850)
    lens, plens = [285, 200, 120, 60], [150, 100, 75, 40]
    L, P = max(lens), max(plens)
    src = torch.tensor(lens)
    pad = torch.arange(L)[None, :] >= src[:, None]
    texts = torch.randint(1, 300, (4, L), generator=g).masked_fill(pad, 0)
    prompts = torch.randint(0, PAD, (4, 6, P), generator=g)
    for u, n in enumerate(plens):
        prompts[u, :, n:] = PAD
    fx = golden("flamed_sample")
    fp = t32(fx["prompts"]).clone()
    fp[1, :, 13:] = PAD
    return {"a": (texts, src, prompts, plens, 64),
            "fixture": (t32(fx["phonemes"]), t32(fx["src_lens"]), fp, [20, 13], 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--dump", default="")
    ap.add_argument("--compare", default="")
    ap.add_argument("--persist", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prior_exact_time.py measures on the GPU; no device found")
    from _flamed_common import build_flamed
    from flamed import _native as nat
    from flamed.utils.tools import get_mask_from_lengths
    dev = torch.device("cuda:0")
    pg = build_flamed(dev, "bf16")[0].prior_generator
    base = {"label": args.label, "lib": os.path.relpath(nat.LIB_PATH, REPO)}
    dumped, spread = {}, 0.0

    def emit(batch, what, r):
        nonlocal spread
        if "median_ms" in r:
            spread = max(spread, (r["max_ms"] - r["min_ms"]) / r["median_ms"])
        print(json.dumps({**base, "batch": batch, "what": what, **r}), flush=True)

    with torch.inference_mode():
        for name, (texts, src, prompts, plens, nfe) in batches().items():
            texts, src, prompts = texts.to(dev), src.to(dev), prompts.to(dev)
            B, L = texts.shape
            P = prompts.shape[-1]
            mask = get_mask_from_lengths(src, L)
            enc = pg.hip().encode(texts, mask)
            lens = src.tolist()

            def stage(exact, e=enc, s=src, m=mask, pr=prompts, pl=plens, p=P):
                torch.manual_seed(11)
                x, tl = pg.pva.sample(e, s, m, nfe=nfe, temperature=0.3, exact=exact) if exact else \
                    pg.pva.sample(e, s, m, nfe=nfe, temperature=0.3)
                tm = get_mask_from_lengths(tl, x.size(1))
                return (pg.hip().decode(x, tm, pr, p, prompt_lens=pl) if exact else pg.hip().decode(x, tm, pr, p)), tl

            def flow_only(exact):
                torch.manual_seed(11)
                return pg.pva.flow(enc, mask, nfe, 0.3, exact=True) if exact else pg.pva.flow(enc, mask, nfe, 0.3)

            def alone():
                out = []
                for u, n in enumerate(lens):
                    out.append(stage(False, enc[u:u + 1, :n].contiguous(), src[u:u + 1], mask[u:u + 1, :n].contiguous(),
                                     prompts[u:u + 1, :, :plens[u]].contiguous(), None, plens[u]))
                return out

            emit(name, "dense", timed(lambda: stage(False), args.reps, args.warmup, dev))
            emit(name, "dense_flow", timed(lambda: flow_only(False), args.reps, args.warmup, dev))
            if args.dump or args.compare:
                d, s = flow_only(False)
                (pe, lg), tl = stage(False)
                dumped.update({f"{name}_{k}": v.cpu().numpy() for k, v in
                               (("dur", d), ("sil", s), ("tgt_len", tl), ("prior_embs", pe), ("logits", lg))})
            if args.dense_only:
                continue
            r0 = pg.pva.hip().persist_status()[0]
            emit(name, "exact", timed(lambda: stage(True), args.reps, args.warmup, dev))
            emit(name, "exact_flow", timed(lambda: flow_only(True), args.reps, args.warmup, dev))
            if args.persist:
                emit(name, "persist", {"exact_flows": 2 * (args.reps + args.warmup),
                                       "persistent_launches": pg.pva.hip().persist_status()[0] - r0})
            emit(name, "alone", timed(alone, args.reps, args.warmup, dev))
            emit(name, "dense", timed(lambda: stage(False), args.reps, args.warmup, dev))
            (_, _), tx = stage(True)
            (_, _), td = stage(False)
            emit(name, "frames", {"exact_tgt_len": tx.tolist(), "dense_tgt_len": td.tolist(),
                                  "alone_tgt_len": [int(o[1][0]) for o in alone()]})
    emit("-", "spread", {"largest_max_minus_min_over_median": round(spread, 4)})
    if args.dump:
        np.savez(args.dump, **dumped)
    if args.compare:
        with np.load(args.compare) as z:
            same = {k: bool(np.array_equal(z[k], dumped[k])) for k in z.files}
        emit("-", "bitwise_vs_" + os.path.basename(args.compare), same)


if __name__ == "__main__":
    main()
