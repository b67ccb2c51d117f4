"""Prompt-side RVQ and timbre encoder on HIP (csrc/prompt.hip, flamed_vq_encode) against the fp64 oracle, per row and per
frame (tests/_promptprofile.py), f32.

The timbre encoder is the one user of attn_kernel<64>, attn_mfma_kernel<64, 4>, ln_mask_kernel<256> and the k = 5
LoadConvRows GEMM (K = 1280); its last-LayerNorm rows are read from the handle's workspace (flamed_vq_ws_offsets,
include/flamed_diag.h), so a wrong row is seen before mean_t_kernel averages it away.

  rows, spk      no row further from the fp64 oracle than min(4 x the fp32 oracle's worst row of that case, 1e-5); spk
                 the same against its own floor; attn_mfma 1 and 0
  codes          bit-exact against the fp32 oracle; only a frame whose first mismatching layer sits on an oracle top-2
                 gap below 1e-5 is excused, none at T <= 481, and never more cells than the oracle's own near-ties
  outs, qbuf[g]  per frame against the fp64 rvq_quantize on every frame whose six codes equal the fp64 oracle's (at most
                 0.5 % excluded), bar min(4 x the frame floor, 1e-5)
  ties           codebooks of exact duplicates placed in one thread, in neighbouring lanes, in two waves: the lowest
                 index wins wherever the oracle's gap to a different row is at least 1e-5
  batch isolation, graph replay == eager, shape sequences on the one-buffer-set handle, strided input: bitwise

Shapes: _promptprofile.SHAPES (what each reaches is written there).  Floors come from the oracle alone."""
import ctypes

import pytest
import torch

import _promptprofile as pp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("codes", "outs", "qbuf", "rows", "spk")


def _build(sd):
    from flamed.models.facodec import FACodecDecoder
    d = FACodecDecoder(in_channels=256, upsample_initial_channel=1024, up_ratios=[5, 5, 4, 2], vq_dim=256).eval()
    d.load_state_dict(sd)
    d.hip_dtype = "f32"
    return d.to(DEV)


@pytest.fixture(scope="module")
def dec():
    return _build(pp.decoder_sd())


@pytest.fixture(scope="module")
def fresh():
    """A second handle of the same weights, for eager runs that share no buffers or graph with `dec`."""
    return _build(pp.decoder_sd())


@pytest.fixture(scope="module")
def tied():
    built = {}

    def get(kind):
        if kind not in built:
            sd = pp.memo("prompt_tied_sd", lambda: pp.tied_state_dicts(pp.decoder_sd()))[kind]
            built[kind] = (_build(sd), sd)
        return built[kind]
    return get


def _tune(**knobs):
    from flamed import _native as nat
    for k, v in knobs.items():
        nat.check(nat.lib().flamed_tune(k.encode(), int(v)), "flamed_tune")


def _run(d, xd, graph=True):
    """One flamed_vq_encode of a device input (B, 256, T) -> CPU {codes, outs, qbuf (G, B, 256, T), rows (B, T, 256),
    spk}; the rows are the workspace's H buffer, which mean_t_kernel has just averaged."""
    from flamed import _native as nat
    B, _, T = xd.shape
    d.hip_graph = graph
    try:
        with torch.inference_mode():
            outs, codes, _, qb, spk = d(xd, eval_vq=False, vq=True)
            h = d._vq_hip
            assert h is not None and h.handle is not None  # the HIP path ran
            off = (ctypes.c_size_t * 6)()
            nat.check(nat.lib().flamed_vq_ws_offsets(h.handle, B, T, off), "flamed_vq_ws_offsets")
            assert off[2] + 4 * B * T * 256 <= h.ws.buf.numel()
            rows = h.ws.buf[off[2]:off[2] + 4 * B * T * 256].view(torch.float32).view(B, T, 256).clone()
    finally:
        d.hip_graph = True
    return {"codes": codes.cpu(), "outs": outs.cpu(), "qbuf": torch.stack(list(qb)).cpu(), "rows": rows.cpu(),
            "spk": spk.cpu()}


def _same(a, b, what, sel=None):
    for k in KEYS:
        u, v = a[k], b[k]
        if sel is not None:  # utterance axis: codes (n_q, B, T), qbuf (G, B, C, T), the others (B, ...)
            ax = 1 if k in ("codes", "qbuf") else 0
            u, v = u.index_select(ax, sel), v.index_select(ax, sel)
        assert u.shape == v.shape and torch.equal(u, v), f"{what}: {k} differs"


# ------------------------------------------------------------------------------------------------------------
# profiles at the edge shapes
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("attn_mfma", [1, 0])
@pytest.mark.parametrize("B,T", pp.SHAPES, ids=lambda v: str(v))
def test_rows_and_spk(dec, B, T, attn_mfma):
    x, r = pp.case(B, T)
    try:
        _tune(attn_mfma=attn_mfma)
        o = _run(dec, x.to(DEV))
    finally:
        _tune(attn_mfma=1)
    f = pp.floors(r)
    assert torch.isfinite(o["rows"]).all() and torch.isfinite(o["spk"]).all()
    e = pp.row_err(o["rows"], r["r64"]["rows"])
    se = float(pp.spk_err(o["spk"], r["r64"]["spk"], r["r64"]["rows"]).max())
    emax, at = float(e.max()), int(e.argmax())
    print(f"prompt rows ({B}, {T}) attn_mfma={attn_mfma}: row max {emax:.3e} (utterance {at // T}, row {at % T}), floor "
          f"{f['rows']:.3e}, ratio {emax / f['rows']:.2f}, median {float(e.median()):.3e}; spk {se:.3e}, floor "
          f"{f['spk']:.3e}, ratio {se / f['spk']:.2f}")
    assert emax <= pp.bar_of(f["rows"]), (f"row {at % T} of utterance {at // T} is {emax:.3e} from the fp64 oracle, "
                                         f"{emax / f['rows']:.2f}x the floor {f['rows']:.3e}")
    assert se <= pp.bar_of(f["spk"]), f"spk is {se:.3e} from the fp64 oracle, {se / f['spk']:.2f}x the floor {f['spk']:.3e}"


@pytest.mark.parametrize("B,T", pp.SHAPES, ids=lambda v: str(v))
def test_codes_and_quantized(dec, B, T):
    x, r = pp.case(B, T)
    o = _run(dec, x.to(DEV))
    r32, r64 = r["r32"], r["r64"]
    codes = o["codes"]
    assert codes.shape == r32["codes"].shape and codes.dtype == torch.int64
    near = r32["gaps"] < pp.NEAR_TIE
    neq = codes != r32["codes"]
    first = neq & (neq.float().cumsum(0) == 1)  # a frame's first mismatching layer; later ones follow from it
    print(f"prompt codes ({B}, {T}): {int(neq.sum())} cells differ, {int(first.sum())} first mismatches, oracle "
          f"near-ties {int(near.sum())} of {near.numel()}")
    if T <= 481:
        assert not bool(neq.any()), "code mismatch (no near-tie excuse at T <= 481)"
    assert bool((near | ~first).all()), "code mismatch away from a near-tie"
    assert int(first.sum()) <= int(near.sum()), "more excused cells than the oracle has near-ties"
    keep = (codes == r64["codes"]).all(0)
    excluded = int((~keep).sum())
    assert excluded <= 0.005 * B * T, f"{excluded} of {B * T} frames excluded"
    f = pp.floors(r)
    for name, out, ref, fl in [("outs", o["outs"], r64["outs"], f["outs"])] + \
            [(f"qbuf[{g}]", o["qbuf"][g], r64["qbuf"][g], f["qbuf"][g]) for g in range(3)]:
        assert out.shape == ref.shape and torch.isfinite(out).all()
        e = pp.frame_err(out, ref, keep)
        emax, at = float(e.max()), int(e.argmax())
        print(f"prompt {name} ({B}, {T}): frame max {emax:.3e} (utterance {at // T}, frame {at % T}), floor {fl:.3e}, "
              f"ratio {emax / fl:.2f}, excluded {excluded}")
        assert emax <= pp.bar_of(fl), (f"{name}: frame {at % T} of utterance {at // T} is {emax:.3e} from the fp64 oracle, "
                                      f"{emax / fl:.2f}x the floor {fl:.3e}")


@pytest.mark.parametrize("B,T", [(2, 65), (1, 193)])
@pytest.mark.parametrize("kind", pp.TIE_KINDS)
def test_exact_ties_take_the_lowest_index(tied, kind, B, T):
    """Every winner has an exact copy at a higher index, held by the same thread ("thread": the strict > of the scan),
    a neighbouring lane ("lane": the shuffle butterfly's index compare) or another wave ("wave": the LDS merge)."""
    d, sd = tied(kind)
    x = pp.case_input(B, T)

    def ref():
        with torch.inference_mode():
            return pp.orc.decoder_vq(sd, x)[0], pp.gap_excluding_copies(sd, x)
    rc, gap = pp.memo(("prompt_tie", kind, B, T), ref)
    codes = _run(d, x.to(DEV))["codes"]
    clear = gap >= pp.NEAR_TIE
    bad = (codes != rc) & clear
    print(f"prompt ties {kind} ({B}, {T}): {int((codes != rc).sum())} cells differ, {int(clear.sum())} of {clear.numel()} "
          f"judged, higher index of a pair returned on {int(pp.higher_of_pair(kind, codes).sum())}")
    assert not bool(bad.any()), f"{int(bad.sum())} cells differ from the oracle; higher index of a pair on " \
                                f"{int((pp.higher_of_pair(kind, codes) & clear).sum())}"


# ------------------------------------------------------------------------------------------------------------
# isolation, replay, stale state, strides: bitwise
# ------------------------------------------------------------------------------------------------------------

def test_batch_isolation(dec):
    B, T = 3, 65
    x = pp.case_input(B, T)
    xb = x.clone()
    xb[1] = pp.case_input(B, T, 1)[1]
    a, b = _run(dec, x.to(DEV)), _run(dec, xb.to(DEV))
    assert not torch.equal(a["rows"][1], b["rows"][1]) and not torch.equal(a["codes"][:, 1], b["codes"][:, 1])
    _same(a, b, "an utterance changed with its neighbour", torch.tensor([0, 2]))


@pytest.mark.parametrize("B,T", [(1, 1), (3, 161)])
def test_graph_replay_equals_eager(dec, B, T):
    xd = pp.case_input(B, T).to(DEV)
    eager = _run(dec, xd, graph=False)
    g1 = _run(dec, xd)
    g2 = _run(dec, xd)
    _same(eager, g1, "graph replay against eager")
    _same(g1, g2, "second replay")


def test_shape_sequence_no_stale_state(dec, fresh):
    """(2, 96) -> (3, 64) -> (2, 96) -> (1, 1) -> (2, 96) on one handle with the graph on; the handle keeps one buffer
    set, and the first steps have equal element counts, so freed buffers and the workspace may come back at the same
    addresses under another shape.  Every step equals an eager run of its input on a second handle."""
    for i, (B, T) in enumerate([(2, 96), (3, 64), (2, 96), (1, 1), (2, 96)]):
        xd = pp.case_input(B, T, s=i).to(DEV)
        _same(_run(dec, xd), _run(fresh, xd, graph=False), f"step {i} ({B}, {T})")


def test_strided_input(dec):
    B, T = 2, 65
    xt = pp.case_input(B, T).transpose(1, 2).contiguous().to(DEV)  # (B, T, C)
    view = xt.transpose(1, 2)
    assert not view.is_contiguous()
    _same(_run(dec, view), _run(dec, view.contiguous()), "transposed view against its contiguous copy")
