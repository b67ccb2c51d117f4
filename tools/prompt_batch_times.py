#!/usr/bin/env python
"""Times of the prompt stage for a batch of distinct prompts (DESIGN.md "Exact lengths", "Prompt stage";
profiles/prompt_lens_times.txt).

f32 encoder handle (the default: the codes need it), calm encoder weights (weight-norm gains x the `facodec_calm` gain),
the seeded prompt-side decoder.  Every figure is wall clock from a device sync to the arrival of the codes and timbres on
the host, the median (min .. max) of --reps calls after --warmup calls, the ways alternating within one process:

  solo          the parent's way (synthesize.encode_prompt_features): per prompt one FACodecEncoder call, one
                FACodecDecoder(vq=True) call and one device-to-host copy, one prompt after another
  solo_nograph  the same with hip_graph off (one handle keeps one dense graph, so prompts of different lengths re-capture
                on every call)
  batch         one ragged call pair with exact lengths and one copy (Flamed.encode_prompts does the same two calls)
  batch_noskip  the same with the tile skip off (flamed_tune("enc_skip", 0)); timed in a block of its own against `solo`
                again, because a knob change re-captures every graph

Batches: four prompts of 3 s; four of 3 / 5 / 7 / 10 s; sixteen of mixed length (seeded, 2 .. 10 s).  --solo-only is
all a library without the lens entry points can do: run it with FLAMED_HIP_LIB pointing at a build of the parent commit,
alternated with runs of this build.  One JSON line per figure on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "flamed-tts_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SR = 16000


def batches():
    g = torch.Generator().manual_seed(16)
    mixed = [int(SR * s) for s in (2 + 8 * torch.rand(16, generator=g)).tolist()]
    return {"4x3s": [3 * SR] * 4, "4x3-5-7-10s": [3 * SR, 5 * SR, 7 * SR, 10 * SR], "16xmixed": mixed}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solo-only", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prompt_batch_times.py measures on the GPU; no device found")
    import _promptlens as pl
    from flamed import _native as nat
    dev = torch.device("cuda:0")
    enc, dec = pl.make_encoder("f32", dev), pl.make_decoder(dev)

    def solo(wavs):
        out = []
        for w in wavs:
            _, codes, _, _, spk = dec(enc(w), eval_vq=False, vq=True)
            out.append((codes.permute(1, 0, 2).contiguous().squeeze(0).cpu(), spk.squeeze(0).cpu()))
        return out

    def batch(wav, lens, frames):
        _, codes, _, _, spk = dec(enc(wav, lens=lens), eval_vq=False, vq=True, lens=frames, pad_code=pl.PAD)
        return torch.cat([codes.reshape(-1).float(), spk.reshape(-1)]).cpu()  # one copy

    def once(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def alternate(ways):
        """{name: fn} -> {name: [ms]}: warm every way, then --reps rounds of one call of each in turn."""
        for fn in ways.values():
            for _ in range(args.warmup):
                fn()
        ms = {k: [] for k in ways}
        for _ in range(args.reps):
            for k, fn in ways.items():
                ms[k].append(once(fn))
        return ms

    def graph_off(fn):
        def run():
            enc.hip_graph = dec.hip_graph = False
            try:
                fn()
            finally:
                enc.hip_graph = dec.hip_graph = True
        return run

    for name, lens in batches().items():
        n = max(lens)
        gen = torch.Generator().manual_seed(n + len(lens))
        wav = torch.zeros(len(lens), 1, n)
        for u, m in enumerate(lens):
            wav[u, 0, :m] = 0.1 * torch.randn(m, generator=gen)
        wavd = wav.to(dev)
        wavs = [wavd[u:u + 1, :, :m].contiguous() for u, m in enumerate(lens)]
        frames = [pl.out_len(m) for m in lens]
        base = {"label": args.label, "lib": os.path.relpath(nat.LIB_PATH, REPO), "batch": name, "B": len(lens),
                "seconds": [round(m / SR, 2) for m in lens], "padding_rows": round(1 - sum(lens) / (n * len(lens)), 3)}

        def emit(what, v):
            print(json.dumps({**base, "what": what, "median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                              "max_ms": round(max(v), 3), "reps": len(v)}), flush=True)

        with torch.inference_mode():
            ways = {"solo": lambda: solo(wavs), "solo_nograph": graph_off(lambda: solo(wavs))}
            if not args.solo_only:
                ways["batch"] = lambda: batch(wavd, lens, frames)
            for k, v in alternate(ways).items():
                emit(k, v)
            if args.solo_only:
                continue
            nat.check(nat.lib().flamed_tune(b"enc_skip", 0), "flamed_tune")
            try:
                for k, v in alternate({"solo": lambda: solo(wavs), "batch_noskip": lambda: batch(wavd, lens, frames)}).items():
                    emit(k + ("_again" if k == "solo" else ""), v)
            finally:
                nat.check(nat.lib().flamed_tune(b"enc_skip", 1), "flamed_tune")


if __name__ == "__main__":
    main()
