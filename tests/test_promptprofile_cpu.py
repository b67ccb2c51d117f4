"""CPU calibration of the prompt-stage profiles (tests/_promptprofile.py): the emulation is the oracle bitwise, the
fp32 oracle's floors and near-tie counts on the GPU suite's shapes, planted bugs against the row / spk bars, and the
tied codebooks.  No GPU, no HIP library."""
import pytest
import torch

from _common import orc, rel_l2
import _promptprofile as pp

MARGIN = 1.5      # every planted bug must stand this far above the bar it is judged by (tests/_xfmrprofile.py)
OLD_BAR = 1e-4    # test_vq_timbre_vs_oracle's global figure: spk rel-L2
SEEDS = (0, 1)


@pytest.fixture(scope="module")
def sd():
    return pp.decoder_sd()


@pytest.mark.parametrize("B,T", [(1, 1), (3, 5), (2, 65), (3, 161)])
def test_identity_emulation_is_the_oracle(sd, B, T):
    x = pp.case_input(B, T).transpose(1, 2)
    with torch.inference_mode():
        ref = orc.timbre_encoder(sd, x)
        assert torch.equal(pp.emulated_timbre(sd, x), ref)
        assert torch.equal(pp.emulated_timbre(sd, x, mutate=lambda s, v, c: v), ref)
        assert torch.equal(pp.spk_of(ref), orc.decoder_vq(sd, x.transpose(1, 2))[1])


def test_error_definitions():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(2, 5, 256, generator=g, dtype=torch.float64)
    out = ref.clone()
    out[1, 3] += 1e-3 * torch.randn(256, generator=g, dtype=torch.float64)
    e = pp.row_err(out, ref)
    rms = ref.reshape(-1, 256).pow(2).sum(1).mean().sqrt()
    assert e.shape == (10,) and int(e.argmax()) == 8 and float((e > 0).sum()) == 1
    assert abs(float(e[8]) - float((out[1, 3] - ref[1, 3]).norm() / rms)) < 1e-15
    s = pp.spk_err(ref.mean(1) + 1e-3, ref.mean(1), ref)
    assert torch.allclose(s, torch.full((2,), 1e-3 * 16.0 / float(rms), dtype=torch.float64))
    keep = torch.ones(2, 5, dtype=torch.bool)
    keep[1, 3] = False
    assert float(pp.frame_err(out.transpose(1, 2), ref.transpose(1, 2), keep).max()) == 0.0
    assert float(pp.frame_err(out.transpose(1, 2), ref.transpose(1, 2)).max()) > 0.0


# ------------------------------------------------------------------------------------------------------------
# floors, code agreement and near-ties of the GPU suite's inputs
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", SEEDS)
@pytest.mark.parametrize("B,T", pp.SHAPES, ids=lambda v: str(v))
def test_floors_codes_and_near_ties(B, T, s):
    """Per case: the fp32 oracle's codes equal the fp64 oracle's on every cell; its floors (printed; the ranges are in
    the helper's docstring) stay under the cap, so the bar is 4 x the floor everywhere; and the inputs' near-ties:
    the share of (layer, frame) cells with an fp32 top-2 gap below 1e-5 is at most 0.1 %, and 0 for T <= 481."""
    _, r = pp.case(B, T, s)
    assert torch.equal(r["r32"]["codes"], r["r64"]["codes"])
    f = pp.floors(r)
    near = int((r["r32"]["gaps"] < pp.NEAR_TIE).sum())
    cells = r["r32"]["gaps"].numel()
    print(f"prompt floor ({B}, {T}) s={s}: rows max {f['rows']:.2e} median {f['rows_median']:.2e}, spk {f['spk']:.2e}, "
          f"outs {f['outs']:.2e}, qbuf {' '.join(f'{q:.2e}' for q in f['qbuf'])}; near-ties {near} of {cells}")
    for v in [f["rows"], f["spk"], f["outs"]] + f["qbuf"]:
        assert 0 < pp.FACTOR_F32 * v < pp.F32_ROW_BAR
    assert near <= 1e-3 * cells
    if T <= 481:
        assert near == 0


# ------------------------------------------------------------------------------------------------------------
# planted bugs
# ------------------------------------------------------------------------------------------------------------

def _at(site, fn, layer=None):
    def mutate(s, v, ctx):
        if s != site or (layer is not None and ctx["layer"] != layer):
            return v
        v = v.clone()
        r = fn(v, ctx)
        return v if r is None else r
    return mutate


def _bugs(B, T):
    NI = float("-inf")

    def last_key(v, c):
        v[1, 2, 80, T - 1] = NI

    def group_key(v, c):
        v[1, :, 0:64, 64] = NI

    def cross(v, c):
        c["leak"].append((1, 80, 2, 0))

    def tap_m1_leak(v, c):
        k = c["w"].shape[-1]
        v[1, :, 0] += c["w"][:, :, k // 2 - 1] @ c["x"][0, :, T - 1]

    def lose_tap_p2(v, c):
        k = c["w"].shape[-1]
        v[1, :, T - 3] -= c["w"][:, :, k // 2 + 2] @ c["x"][1, :, T - 1]

    def lose_tap_m2(v, c):
        k = c["w"].shape[-1]
        v[1, :, T - 1] -= c["w"][:, :, k // 2 - 2] @ c["x"][1, :, T - 3]

    def mean_t1(v, c):
        return v * (T / (T + 1.0))

    def pe0(v, c):
        v[1] = pp.emulated_timbre(c["sd"], c["x"][1:2])[0]  # alone, utterance 1 gets pe[:1]
    return [("query 80 of utt 1 loses its last key, head 2, layer 0", _at("att", last_key, 0)),
            ("the same in layer 3", _at("att", last_key, 3)),
            ("queries 0..63 of utt 1 lose key 64 (first of key group 1), all heads, layer 0", _at("att", group_key, 0)),
            ("query 80 of utt 1 attends key 0 of utt 2, layer 0", _at("att", cross, 0)),
            ("frame 0 of utt 1 reads utt 0's last frame through tap -1, layer 0", _at("conv", tap_m1_leak, 0)),
            ("frame T-3 of utt 1 loses tap +2 (its last frame), layer 0", _at("conv", lose_tap_p2, 0)),
            ("frame T-1 of utt 1 loses tap -2, layer 0", _at("conv", lose_tap_m2, 0)),
            ("the mean divides by T + 1", _at("spk", mean_t1)),
            ("utterance 1 is encoded with pe[0]", _at("rows", pe0))]


def test_last_frame_tap_plus_2_reads_padding(sd):
    """Tap +2 of an utterance's last frame lies in the reference's zero padding: there is nothing for a kernel to
    lose, so the planted edge bugs are its two real neighbours (frame T-3's tap +2, the last frame's tap -2)."""
    w = sd["timbre_encoder.layers.0.ffn.ffn_1.weight"]
    x = torch.randn(1, 256, 9, generator=torch.Generator().manual_seed(0))
    y = torch.nn.functional.conv1d(x, w, padding=2)
    z = torch.nn.functional.conv1d(torch.cat([x, torch.zeros(1, 256, 2)], 2), w, padding=2)
    assert torch.equal(y[:, :, 8], z[:, :, 8])


def test_planted_bugs_against_the_bars(sd):
    B, T = 3, 161
    x, r = pp.case(B, T)
    r64 = r["r64"]
    f = pp.floors(r)
    rbar, sbar = pp.bar_of(f["rows"]), pp.bar_of(f["spk"])
    print(f"\nplanted bugs at ({B}, {T}): row floor {f['rows']:.2e} bar {rbar:.2e}; spk floor {f['spk']:.2e} bar {sbar:.2e}")
    print(f"  {'bug':<82} {'row max':>9} {'x floor':>8} {'x bar':>8} {'spk err':>9} {'x bar':>8}  spk rel-L2 (old {OLD_BAR:g})")
    passed_old = []
    with torch.inference_mode():
        for label, mut in _bugs(B, T):
            rows = pp.emulated_timbre(sd, x.transpose(1, 2), mutate=mut)
            spk = pp.spk_of(rows, mutate=mut)
            e = float(pp.row_err(rows, r64["rows"]).max())
            se = float(pp.spk_err(spk, r64["spk"], r64["rows"]).max())
            old = rel_l2(spk, r64["spk"])
            print(f"  {label:<82} {e:9.2e} {e / f['rows']:8.1e} {e / rbar:8.1e} {se:9.2e} {se / sbar:8.1e}  "
                  f"{old:.2e} {'passed' if old < OLD_BAR else 'failed'}")
            if old < OLD_BAR:
                passed_old.append(label)
            if label.startswith("the mean"):
                assert se >= MARGIN * sbar, label     # the rows are right: only the embedding can show it
            else:
                assert e >= MARGIN * rbar, f"{label}: row max {e:.3e} under {MARGIN} x the bar {rbar:.3e}"
    # what the global figure alone let through: a single query's lost or foreign key, in any layer
    assert len(passed_old) >= 3, passed_old


# ------------------------------------------------------------------------------------------------------------
# exact ties
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", [(2, 65), (1, 193)])
@pytest.mark.parametrize("kind", pp.TIE_KINDS)
def test_tied_codebooks(sd, kind, B, T):
    """Every codebook row has an exact copy: the oracle (torch.max: first index) never returns the higher index of a
    pair, its plain top-2 gap is exactly 0 on more than half of the cells ("thread" and "lane": on every cell), and
    the gap that excludes copies is what separates the winner from a different row."""
    tsd = pp.tied_state_dicts(sd)[kind]
    x = pp.case_input(B, T)
    with torch.inference_mode():
        gaps = []
        codes, _ = orc.decoder_vq(tsd, x, gaps=gaps)
    gaps = torch.stack(gaps)
    assert not bool(pp.higher_of_pair(kind, codes).any())
    tied = float((gaps == 0).float().mean())
    ex = pp.gap_excluding_copies(tsd, x)
    print(f"tied codebooks {kind} ({B}, {T}): exact ties on {100 * tied:.1f} % of cells; gap excluding copies min "
          f"{float(ex.min()):.2e}, cells under 1e-5: {int((ex < pp.NEAR_TIE).sum())} of {ex.numel()}")
    assert tied > 0.5
    if kind in ("thread", "lane"):
        assert tied == 1.0
    assert ex.shape == codes.shape and bool((ex >= 0).all()) and bool((ex >= gaps).all())
    # on the untied weights nothing is a copy: the two gaps agree
    g0 = []
    orc.decoder_vq(sd, x, gaps=g0)
    assert torch.equal(pp.gap_excluding_copies(sd, x), torch.stack(g0))
