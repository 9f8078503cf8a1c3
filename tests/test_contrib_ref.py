"""The float64 windows of the blend-contribution statistics (tests/dense_contrib64.py) proved on the CPU before anything runs on a GPU: a
float32 emulation of siu3r_raster_contrib in the kernel's own definitions (the decisions of dense_raster_bwd64._walk(f32=True)) lies
inside every window of every composite case of both families, the windows are narrow enough to check something, the new crafted cases
keep the share of undecided pixels within ZERO_SHARE_CAP, and each wrong answer of dense_contrib64.MUTATIONS falls outside a window."""
import numpy as np
import pytest

import dense_contrib64 as K
import dense_raster_fwd64 as F


@pytest.mark.parametrize("name", K.ALL_NAMES)
def test_emulation_inside_every_window(name):
    c = K.contrib_case(name)
    wmax, count, wsum = K.contrib_emul32(c)
    worst = K.check_contrib(name, c, wmax, count, wsum)
    print(f"[contrib ref] {name}: worst wsum error {worst:.3f} of its tolerance")
    blended = sum(int((r["count_lo"] > 0).sum()) for r in K.contrib_ref(c))
    assert blended > 0, f"{name}: nothing blends"


@pytest.mark.parametrize("name", K.NEW_NAMES)
def test_new_cases_are_what_they_claim(name):
    c = K.contrib_case(name)
    refs = K.contrib_ref(c)
    if c["scene"] == "crowd":
        assert c["G"] > F.STG
        passes = np.ones(len(c["bins"][0][1]), bool)  # one tile, one bin: every entry covers it
        rounds, walks = F.refill_rounds(passes)
        assert walks >= 2, (rounds, walks)
        assert all((r["count_lo"] > 0).all() for r in refs), "every Gaussian of the crowd blends somewhere"
    else:
        assert (c["W"], c["H"], c["V"]) == (40, 24, 2) and 64 <= c["G"] <= 96
    if c["scene"] == "span4":  # some row blends in all four tiles around (16, 16)
        ts, ids = c["lists"][0]
        tiles_of = lambda g: {t for t in range(len(ts) - 1) if g in ids[ts[t]:ts[t + 1]]}
        assert any(tiles_of(g) >= {0, 1, 3, 4} for g in range(c["G"]))
    if c["scene"] in ("wall", "culled"):
        assert c["zero_rows"][0].any()
        for v, r in enumerate(refs):
            assert (r["count_hi"][c["zero_rows"][v]] == 0).all() and (r["wmax_hi"][c["zero_rows"][v]] == 0).all(), "the reference itself blends a hidden row"
    if c["scene"] == "clamp":
        on_clamp = sum(int((w["bl"] & w["clamped"]).sum()) for r in F.comp_fwd_ref(c) for w in r["walks"].values())
        assert on_clamp > 0


# the wrong answers, each on the smallest case that shows it
WRONG = {"post_blend_T": "k2_span4", "no_alpha_max": "k2_clamp", "count_saturating": "k2_wall", "alpha_only": "k3_span4", "no_tile_merge": "k2_span4",
         "no_half": "k3_clamp"}


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_wrong_answers_fall_outside_a_window(mutation):
    name = WRONG[mutation]
    c = K.contrib_case(name)
    with pytest.raises(AssertionError):
        K.check_contrib(name, c, *K.contrib_emul32(c, mutate=mutation))
