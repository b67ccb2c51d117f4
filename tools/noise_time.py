"""Time ProbGenerator.sample with the reference's noise (seeds=None: torch.randn on the CPU from the global RNG plus a
pageable host-to-device copy -- the parent's code path, the baseline) and with keyed noise (seeds=: one HIP kernel,
flamed_noise_state), e.g.
    python tools/noise_time.py --reps 20
Workloads: B = 1 x 400 at 128 Euler evaluations and at 16 midpoint evaluations, 4 x 800/611/437/250 with exact lengths,
64 x 400.  Per workload and mode one line: the median over --reps timed calls after --warm warm ones of the wall time
around a synchronised call and of the stream time between two events around it (the host's draw and copy keep the
stream idle, so they show in both), with the spread (min .. max) of each.  Last, the noise kernel alone at
64 x 400 x 256 (50 launches captured into one graph, replayed between two events) as bytes/s against the measured
copy peak of DESIGN.md (5.97 TB/s)."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "flamed-tts_amd"))
import torch  # noqa: E402
import yaml  # noqa: E402

COPY_PEAK = 5.97e12  # DESIGN.md "measured peaks": flamed_probe_copy, non-temporal float4
WORKLOADS = [  # (name, lens, nfe, solver, exact_lengths)
    ("B=1 T=400 nfe=128 euler", [400], 128, "euler", False),
    ("B=1 T=400 nfe=16 midpoint", [400], 16, "midpoint", False),
    ("B=4 T=800/611/437/250 nfe=128 euler exact", [800, 611, 437, 250], 128, "euler", True),
    ("B=64 T=400 nfe=128 euler", [400] * 64, 128, "euler", False),
]


def med(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", type=int, default=None, help="index of the one workload to run")
    a = ap.parse_args()
    from flamed.models.synthesizer.prob_generator import ProbGenerator
    from flamed.utils.noise import hip_noise_state, utterance_seeds
    from flamed.utils.seeded_init import randomize_module
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(REPO, "flamed-tts_amd", "configs", "prob.yaml")))
    pg = ProbGenerator(cfg).eval()
    randomize_module(pg, 20251205)
    pg = pg.to(dev)
    for k, (name, lens, nfe, solver, exact) in enumerate(WORKLOADS):
        if a.only is not None and k != a.only:
            continue
        B, T = len(lens), max(lens)
        g = torch.Generator().manual_seed(3)
        cond = torch.randn(B, 6, T, 384, generator=g).to(dev)
        spk = torch.randn(B, 256, generator=g).to(dev)
        mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1).to(dev)
        torch.manual_seed(0)
        res = {}
        for mode, seeds in (("seeds=None", None), ("seeds", utterance_seeds(7, range(B))), ("seeds=None again", None)):
            wall, stream = [], []
            with torch.inference_mode():
                for i in range(a.warm + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    out = pg.sample(cond, spk, mask, nfe=nfe, temperature=0.3, solver=solver, exact_lengths=exact, seeds=seeds)
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= a.warm:
                        wall.append((time.perf_counter() - t0) * 1e3)
                        stream.append(e0.elapsed_time(e1))
            res[mode] = statistics.median(wall)
            print(f"{name} [{mode}]: wall {med(wall)}, stream {med(stream)}, finite {bool(torch.isfinite(out).all())}", flush=True)
        base = min(res["seeds=None"], res["seeds=None again"])
        print(f"{name}: seeds vs seeds=None wall median {res['seeds'] - base:+.3f} ms "
              f"(the two seeds=None runs differ by {abs(res['seeds=None'] - res['seeds=None again']):.3f} ms)", flush=True)
    if a.only is None:
        B, T, C, n = 64, 400, 256, 50
        cond = torch.randn(B, T, C, device=dev)
        out = torch.empty_like(cond)
        seeds = utterance_seeds(7, range(B))
        us = []
        hip_noise_state(cond, seeds, None, 0.3, 0, out=out)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()  # n launches in one captured graph: the host's launch cost stays out
        with torch.cuda.graph(graph, capture_error_mode="relaxed"):
            for _ in range(n):
                hip_noise_state(cond, seeds, None, 0.3, 0, out=out)
        for i in range(a.warm + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warm:
                us.append(e0.elapsed_time(e1) * 1e3 / n)
        nbytes = 2 * B * T * C * 4
        m = statistics.median(us)
        print(f"flamed_noise_state alone {B}x{T}x{C} (with cond): {m:.1f} us per launch ({min(us):.1f} .. {max(us):.1f}), "
              f"{nbytes / 1e6:.1f} MB -> {nbytes / m / 1e6:.2f} TB/s = {100 * nbytes / (m * 1e-6) / COPY_PEAK:.0f} % of the "
              f"measured copy peak ({COPY_PEAK / 1e12:.2f} TB/s)", flush=True)


if __name__ == "__main__":
    main()
