#!/usr/bin/env python
"""Times of the FaCodec decode with exact lengths (DESIGN.md "Exact lengths", profiles/exact_decode_times.txt).

bf16 handle, calm weights (weight-norm gains x the `facodec_calm` gain), (B, T) = (4, 800) with lengths
800 / 611 / 437 / 250 by default -- the shape of the exact-lengths solve's table.  Each figure is the median (min ..
max) of --reps calls of FACodecDecoder.inference between device events, after --warmup calls of the same shape:

  dense    inference(x, spk)                      the padded batch, every utterance over T frames
  ragged   inference(x, spk, lens)                flamed_fac_decode_lens
  alone    inference(x[u:u+1, :, :len_u], ...)    the utterances one after another (one event pair around all B)

--dense-only times the first alone: that is all a library without flamed_fac_decode_lens can do, so a run with
FLAMED_HIP_LIB pointing at a build of the parent commit, alternated with runs of this build, is the check that the
dense path did not move.  --check also compares the ragged result with the utterances decoded alone (bitwise is not
expected: other tile configs) and prints the largest difference.  One JSON line per figure on stdout."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "flamed-tts_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--T", type=int, default=800)
    ap.add_argument("--lens", type=int, nargs="+", default=[800, 611, 437, 250])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fac_lens_time.py measures on the GPU; no device found")
    from _faclens import make_decoder
    from flamed import _native as nat
    dev = torch.device("cuda:0")
    dec = make_decoder(args.dtype, dev)
    B, T, lens = len(args.lens), args.T, list(args.lens)
    g = torch.Generator().manual_seed(800)
    x = torch.randn(B, 256, T, generator=g).to(dev)
    spk = torch.randn(B, 256, generator=g).to(dev)
    base = {"label": args.label, "lib": os.path.relpath(nat.LIB_PATH, REPO), "dtype": args.dtype, "B": B, "T": T, "lens": lens}

    def emit(what, r):
        print(json.dumps({**base, "what": what, **r}), flush=True)

    with torch.inference_mode():
        emit("dense", timed(lambda: dec.inference(x, spk), args.reps, args.warmup, dev))
        if args.dense_only:
            return
        emit("ragged", timed(lambda: dec.inference(x, spk, lens), args.reps, args.warmup, dev))
        slices = [(x[u:u + 1, :, :n].contiguous(), spk[u:u + 1].contiguous()) for u, n in enumerate(lens)]
        # one handle keeps one dense graph: four shapes in turn re-capture on every call, so also without the graph
        emit("alone", timed(lambda: [dec.inference(xu, su) for xu, su in slices], args.reps, args.warmup, dev))
        dec.hip_graph = False
        emit("alone_nograph", timed(lambda: [dec.inference(xu, su) for xu, su in slices], args.reps, args.warmup, dev))
        dec.hip_graph = True
        emit("dense", timed(lambda: dec.inference(x, spk), args.reps, args.warmup, dev))
        if args.check:
            w = dec.inference(x, spk, lens)
            worst = max(float((w[u:u + 1, :, :200 * n] - dec.inference(xu, su)).abs().max())
                        for u, (n, (xu, su)) in enumerate(zip(lens, slices)))
            tail = max(int(torch.count_nonzero(w[u, :, 200 * n:])) for u, n in enumerate(lens))
            print(json.dumps({**base, "what": "check", "max_abs_vs_alone": worst, "nonzero_past_end": tail}), flush=True)


if __name__ == "__main__":
    main()
