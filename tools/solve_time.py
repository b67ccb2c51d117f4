"""Time ProbGenerator solves (the denoiser's Euler loop) for given shapes under knob settings, e.g.
    python tools/solve_time.py --shapes 1x2400x256,2x400x128 --knobs persist=1 persist=0
prints one line per (shape, knob set): median ms per solve over --reps timed solves after a warm one (timed by
itself: the first solve of a shape in the process, which on the launch path captures its graphs), whether the
persistent launch ran, and whether the output equals (bitwise) the shape's first knob set's.
--solver midpoint|heun runs the two-stage second-order solve instead (the shape's last number stays the count of
velocity evaluations).  --make-ref FILE computes, on the CPU in fp32 with the module's own torch ops, a converged
solution (midpoint, --ref-steps steps) of utterance 0 of the one given shape and stores it; --ref FILE then prints
each solve's rel-L2 error of utterance 0 against it (same shape and seeds, so the same inputs).
--lens 800,611,437,250 (one shape, B = the number of lengths, T = the longest) runs the exact-lengths solve of the
padded batch (DenoiserHIP.solve(..., lens=)); --alone then times instead the same utterances solved one after another,
each alone at its own length (the sum is one "solve")."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "flamed-tts_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x2400x256")
    ap.add_argument("--knobs", nargs="*", default=[""])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solver", default="euler", choices=["euler", "midpoint", "heun"])
    ap.add_argument("--lens", default=None)
    ap.add_argument("--alone", action="store_true")
    ap.add_argument("--ref", default=None)
    ap.add_argument("--make-ref", default=None)
    ap.add_argument("--ref-steps", type=int, default=128)
    a = ap.parse_args()
    if a.make_ref:
        return make_ref(a)
    from flamed import _native as nat
    from flamed.models.synthesizer.prob_generator import ProbGenerator
    from flamed.utils.seeded_init import randomize_module
    L = nat.lib()
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(REPO, "flamed-tts_amd", "configs", "prob.yaml")))
    pg = ProbGenerator(cfg).eval()
    randomize_module(pg, 20251205)
    pg = pg.to(dev)
    hip = pg.denoiser.hip()
    defaults = {}
    for shape in a.shapes.split(","):
        B, T, nfe = (int(v) for v in shape.split("x"))
        x0, spk = (v.to(dev) for v in inputs(B, T))
        stage = SOLVERS[a.solver]
        lens = [int(v) for v in a.lens.split(",")] if a.lens else None
        if lens is not None and (len(lens) != B or max(lens) != T):
            raise SystemExit(f"--lens {a.lens}: the shape must be {len(lens)}x{max(lens)}x<nfe>")
        kw = {} if lens is None or a.alone else {"lens": lens}
        if stage is None:
            ts = torch.linspace(0, 1, nfe + 1, device=dev)
            one = lambda x, c: hip.solve(x, ts, c, nfe, **kw)  # noqa: E731
        else:
            tb = torch.linspace(0, 1, nfe // 2 + 1, device=dev)[:-1]
            ts = torch.stack((tb, tb + stage * (1 / (nfe // 2))), dim=1).reshape(-1)
            one = lambda x, c: hip.solve_rk2(x, ts, c, nfe // 2, stage, **kw)  # noqa: E731
        if lens is not None and a.alone:  # every utterance alone at its own length, one after another
            parts = [(x0[u:u + 1, :n].contiguous(), spk[u:u + 1]) for u, n in enumerate(lens)]
            solve = lambda: torch.cat([torch.nn.functional.pad(one(x, c), (0, 0, 0, T - x.shape[1])) for x, c in parts])  # noqa: E731
        else:
            solve = lambda: one(x0, spk)  # noqa: E731
        per = len(lens) if lens is not None and a.alone else 1  # persistent launches of one "solve"
        conv = torch.from_numpy(np.load(a.ref)).double() if a.ref else None
        first = None
        for kn in a.knobs:
            kv = [p.split("=") for p in kn.split(",") if p]
            for k, v in kv:
                nat.check(L.flamed_tune(k.encode(), int(v)), "tune")
            with torch.inference_mode():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = solve()  # the warm one: on the launch path it captures the shape's graphs
                torch.cuda.synchronize()
                warm_ms = (time.perf_counter() - t0) * 1e3
                r0 = hip.persist_status()[0]
                times = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    solve()
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                runs = hip.persist_status()[0] - r0
            if first is None:
                first = ref.clone()
            err = ""
            if runs == a.reps * per and per > 1:
                err = f", persistent kernels {sum(hip.persist_times(a.reps * per)) / a.reps:.3f} ms per {per} solves"
            elif runs == a.reps:  # device time of the persistent launches themselves (HIP events around each kernel)
                dev_ms = statistics.median(hip.persist_times(a.reps))
                err = f", persistent kernel {dev_ms:.3f} ms = {1e3 * dev_ms / nfe:.1f} us per evaluation"
            if conv is not None:
                d = ref[0].double().cpu() - conv
                err += f", rel-L2 of utterance 0 vs the converged solution {float(d.norm() / conv.norm()):.3e}"
            form = "" if lens is None else f" lens {a.lens} ({'each alone' if a.alone else 'exact lengths, one call'})"
            print(f"B={B} T={T} nfe={nfe} {a.solver}{form} [{kn or 'defaults'}]: {statistics.median(times):.2f} ms/solve "
                  f"(min {min(times):.2f}, the warm solve before them {warm_ms:.2f}), "
                  f"persistent launches {runs}/{a.reps}, finite {bool(torch.isfinite(ref).all())}, "
                  f"equal to the first knob set {bool(torch.equal(ref, first))}"
                  f"{err}{chain_info(L, hip)}", flush=True)
            for k, _ in kv:  # back to the process defaults of the Tune struct
                nat.check(L.flamed_tune(k.encode(), defaults.setdefault(k, DEFAULTS.get(k, 0))), "tune")


SOLVERS = {"euler": None, "midpoint": 0.5, "heun": 1.0}


def inputs(B, T):
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(B, T, 256, generator=g) * 0.3 + torch.randn(B, T, 256, generator=g)
    return x0, torch.randn(B, 256, generator=g)


def make_ref(a):
    """Converged solution of utterance 0 (utterances are independent in the denoiser) on the CPU, fp32 torch ops."""
    from flamed.models.synthesizer.prob_generator import ProbGenerator
    from flamed.utils.seeded_init import randomize_module
    B, T, _ = (int(v) for v in a.shapes.split("x"))
    cfg = yaml.safe_load(open(os.path.join(REPO, "flamed-tts_amd", "configs", "prob.yaml")))
    pg = ProbGenerator(cfg).eval()
    randomize_module(pg, 20251205)
    x0, spk = inputs(B, T)
    x, spk = x0[:1].clone(), spk[:1]
    n, ts = a.ref_steps, torch.linspace(0, 1, a.ref_steps + 1)
    dt = 1 / n
    with torch.inference_mode():
        for i in range(n):
            y = x + (0.5 * dt) * pg.denoiser(x, ts[i].reshape(1, 1), spk)
            x = x + dt * pg.denoiser(y, (ts[i] + 0.5 * dt).reshape(1, 1), spk)
    np.save(a.make_ref, x[0].numpy())
    print(f"converged midpoint solution, {n} steps, utterance 0 of B={B} T={T}: {a.make_ref}")


def chain_info(L, hip):
    import ctypes
    if not hasattr(L, "flamed_den_chain_info"):
        return ""
    pk, rt = ctypes.c_int(), ctypes.c_int()
    L.flamed_den_chain_info(hip.handle, ctypes.byref(pk), ctypes.byref(rt))
    return f", chain streams parked {pk.value} (re-created {rt.value})"


DEFAULTS = {"ragged_launch": 1, "persist": 1, "persist_ntw": 8, "persist_multi": 1, "persist_pad": 1, "split_batch": 2, "split_prio": 2, "dwgn": 1, "fuse_euler": 1,
            "persist_opt": 885322, "persist_multi_ntw": 8}

if __name__ == "__main__":
    main()
