#!/usr/bin/env python
"""One sha256 line per output of every stage that shares the exact-lengths idiom (DESIGN.md "Exact lengths: one idiom"),
for fixed seeded inputs: the check that a change to the shared loaders, the length upload or the graph cache leaves every
result bitwise where it was.

Run it once per library in a fresh process each -- this build, and a build of the commit to compare with selected by
FLAMED_HIP_LIB (tools/fac_lens_time.py) -- and diff the two outputs: they must be identical line for line.

Weights as in the tests: calm FaCodec decoder and encoder (weight-norm gains x the `facodec_calm` gain), `seeded(...)`
PVA, prior and prompt-side modules.  f32 and bf16 where the stage has both, graph on and off:

  fac_decode    dense (3, 13), (2, 32); lens (3, 13) 13/7/2, (2, 32) 16/32, (4, 9) 9/1/5/8
  enc_encode    (2, 2400)
  pva_flow      launch and graph path (use_graph 0 and 3): dense (3, 13); exact (3, 13) 13/7/2, (4, 16) 16/15/1/9
  prior_decode  (2, 33, 32) target lengths 33/20: dense, and prompt lengths 32/31
  vq_encode     (2, 240): codes, quantized sum, speaker embedding
  den_solve     (--denoiser) the graph of launches (`persist` knob 0): (B, T, nfe) = (1, 64, 4), (2, 37, 4), (3, 37, 7)
                (odd: no ping-pong fusion), (4, 400, 4) (large-M in-place fused steps); (2, 37, 8) in two parts
                (flamed_den_solve_part, graph_steps 4); midpoint (2, 40, 8) f32 and (4, 400, 8) bf16; exact lengths
                `tiny` and `large` of tests/test_ragged_launch_gpu.SHAPES, and `tiny` with ragged_launch 0

The inputs and models come from the tests' helpers (tests/_faclens.py, _flamed_common.py, _xfmrprofile.py,
test_prior_profile_gpu._decode_inputs, test_denoiser_gpu._prob_gen): a change to those changes the digests, so compare
two libraries with one checkout of this tool and the tests, never digests recorded at different commits.  --denoiser
sets the process knobs `persist`, `graph_steps` and `ragged_launch` and puts each back at its default (1, 16, 1: the
library has no getter): run it in a process of its own, as above.
"""
import argparse
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "flamed-tts_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"


def emit(label, *tensors):
    for i, t in enumerate(tensors):
        t = t.detach().cpu().contiguous()
        h = hashlib.sha256(t.numpy().tobytes()).hexdigest()
        print(f"{label}[{i}] {tuple(t.shape)} {str(t.dtype).replace('torch.', '')} {h}", flush=True)


def both_graphs(obj, label, fn):
    """fn() with obj.hip_graph on, replayed once more, then off."""
    try:
        for graph in (True, True, False):
            obj.hip_graph = graph
            out = fn()
            emit(f"{label} graph={int(graph)}", *(out if isinstance(out, (tuple, list)) else (out,)))
    finally:
        obj.hip_graph = True


def fac_decode():
    from _faclens import inputs, make_decoder
    for mode in ("f32", "bf16"):
        dec = make_decoder(mode, DEV)
        for B, T, lens in ((3, 13, None), (2, 32, None), (3, 13, [13, 7, 2]), (2, 32, [16, 32]), (4, 9, [9, 1, 5, 8])):
            lat, spk = inputs(B, T)
            x, s = lat.to(DEV), spk.to(DEV)
            both_graphs(dec, f"fac_decode {mode} ({B}, {T}) lens={lens}", lambda: dec.inference(x, s, lens))


def enc_encode():
    from _common import golden, seeded
    from _flamed_common import build_codec_encoder
    from flamed.utils.seeded_init import scale_weight_norm_gains
    sd = scale_weight_norm_gains(seeded("facodec_encoder"), float(golden("facodec_calm")["gain"]))
    wav = (0.1 * torch.randn(2, 1, 2400, generator=torch.Generator().manual_seed(2400))).to(DEV)
    for mode in ("f32", "bf16"):
        e = build_codec_encoder("cpu")
        e.load_state_dict(sd)
        e.hip_dtype = mode
        e = e.to(DEV)
        both_graphs(e, f"enc_encode {mode} (2, 2400)", lambda: e(wav))


def pva_flow():
    import yaml
    from _common import PKG, seeded
    from flamed.models.synthesizer.pva import PVA
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "prior.yaml")))["variance_adaptor"]
    m = PVA(cfg).eval()
    m.load_state_dict({k[len("prior_generator.pva."):]: v for k, v in seeded("pva").items()})
    hp = m.to(DEV).hip()
    nfe = 8
    ts = torch.linspace(0, 1, nfe + 1, device=DEV)
    for B, L, lens in ((3, 13, None), (3, 13, [13, 7, 2]), (4, 16, [16, 15, 1, 9])):
        g = torch.Generator().manual_seed(100 * B + L)
        enc = torch.randn(B, L, 192, generator=g).to(DEV)
        d0, s0 = (0.3 * torch.randn(B, L, generator=g)).to(DEV), (0.3 * torch.randn(B, L, generator=g)).to(DEV)
        # the dense flow's padding mask: the same ends as the exact case of this shape
        ends = torch.tensor(lens if lens else [L, L // 2 + 1, 2][:B])
        mask = (torch.arange(L)[None, :] >= ends[:, None]).to(DEV)
        for use_graph in (0, 3, 3):
            emit(f"pva_flow ({B}, {L}) lens={lens} use_graph={use_graph}",
                 *hp._graph_flow(enc, mask, d0, s0, ts, nfe, use_graph, lens))


def prior_decode():
    import _xfmrprofile as xp
    from test_prior_profile_gpu import _decode_inputs
    pg, _ = xp.build_prior(reduced=True)
    pg = pg.to(DEV)
    B, T, P, tl = 2, 33, 32, [33, 20]
    x, _, mask, prompts = _decode_inputs(3, B, T, P, tl)
    prompts = prompts.clamp(max=1023)
    prompts[1, :, 31:] = 1024
    x, mask, prompts = x.to(DEV), mask.to(DEV), prompts.to(DEV)
    try:
        for mode in ("f32", "bf16"):
            pg.hip_dec_dtype = mode
            for plens in (None, [32, 31]):
                both_graphs(pg, f"prior_decode {mode} ({B}, {T}, {P}) tl={tl} plens={plens}",
                            lambda: pg.hip().decode(x, mask, prompts, P, prompt_lens=plens))
    finally:
        pg.hip_dec_dtype = "f32"


def vq_encode():
    from _flamed_common import build_flamed
    _, dec = build_flamed(DEV, "f32")
    x = torch.randn(2, 256, 240, generator=torch.Generator().manual_seed(11)).to(DEV)

    def run():
        outs, codes, _, _, spk = dec(x, eval_vq=False, vq=True)
        return codes, outs, spk
    both_graphs(dec, "vq_encode (2, 240)", run)
    assert dec._vq_hip is not None and dec._vq_hip.handle is not None  # the HIP path ran


def den_solve():
    from flamed import _native as nat
    from test_denoiser_gpu import _prob_gen
    from test_exact_lengths_gpu import _inputs as lens_inputs, _ts
    from test_ragged_launch_gpu import SHAPES
    L = nat.lib()
    tune = lambda key, v: nat.check(L.flamed_tune(key, v), "flamed_tune")
    tune(b"persist", 0)
    try:
        for mode in ("f32", "bf16"):
            pg, _ = _prob_gen(mode)
            hip = pg.denoiser.hip()

            def inputs(B, T):
                g = torch.Generator().manual_seed(1000 * B + T)
                x0 = (0.3 * torch.randn(B, T, 256, generator=g) + torch.randn(B, T, 256, generator=g)).to(DEV)
                return x0, torch.randn(B, 256, generator=g).to(DEV)

            def solves(label, fn):
                hip._ensure(torch.device(DEV))  # creates the handle
                r0 = hip.persist_status()[0]
                both_graphs(pg.denoiser, f"den_solve {mode} {label}", lambda: fn().clone())
                assert hip.persist_status()[0] == r0, "the solve took the persistent path"

            # Euler: fused small-M steps, an odd step count (G = 7: no ping-pong fusion), large-M in-place fused steps
            for B, T, nfe in ((1, 64, 4), (2, 37, 4), (3, 37, 7), (4, 400, 4)):
                x0, spk = inputs(B, T)
                solves(f"({B}, {T}, {nfe})", lambda: hip.solve(x0, torch.linspace(0, 1, nfe + 1, device=DEV), spk, nfe))
            # a solve in two parts (flamed_den_solve_part), four steps per captured graph
            B, T, nfe = 2, 37, 8
            x0, spk = inputs(B, T)
            r = torch.arange(nfe * B, device=DEV)
            mods = hip.adaln(torch.linspace(0, 1, nfe + 1, device=DEV)[:nfe], spk, r // B, r % B)
            ws = torch.empty(L.flamed_den_workspace_size(hip.handle, B, T), dtype=torch.uint8, device=DEV)
            tune(b"graph_steps", 4)
            try:
                for use_graph in (1, 1, 0):
                    x = x0.clone()
                    for s0, s1 in ((0, 4), (4, 8)):
                        nat.check(L.flamed_den_solve_part(hip.handle, nat.ptr(x), nat.ptr(mods), nfe, B, T, nat.ptr(ws), ws.numel(),
                                                          use_graph, s0, s1, nat.stream_ptr(torch.device(DEV))), "flamed_den_solve_part")
                    emit(f"den_solve {mode} ({B}, {T}, {nfe}) parts 0-4-8 graph={use_graph}", x)
            finally:
                tune(b"graph_steps", 16)
            # RK2 (midpoint)
            B, T = (2, 40) if mode == "f32" else (4, 400)
            x0, spk = inputs(B, T)
            solves(f"midpoint ({B}, {T}, 8)", lambda: hip.solve_rk2(x0, _ts(0.5), spk, 4, 0.5))
            # exact lengths on the launch path, and one utterance after another (ragged_launch 0)
            for name, ragged in (("tiny", 1), ("large", 1), ("tiny", 0)):
                lens = SHAPES[name]
                xl, sl = (t.to(DEV) for t in lens_inputs(lens))
                tune(b"ragged_launch", ragged)
                try:
                    solves(f"lens {name} ragged_launch={ragged}", lambda: hip.solve(xl, _ts(None), sl, 8, lens=lens))
                    assert hip.lens_path() == (2 if ragged else 3)
                finally:
                    tune(b"ragged_launch", 1)
    finally:
        tune(b"persist", 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--denoiser", action="store_true", help="also the denoiser's graph of launches")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stage_digest.py runs the library on the GPU; no device found")
    with torch.inference_mode():
        for stage in (fac_decode, enc_encode, pva_flow, prior_decode, vq_encode) + ((den_solve,) if args.denoiser else ()):
            stage()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
