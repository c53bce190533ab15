"""CPU: the cases of tests/beverse_cell_util.py really are what they were chosen for.
  * dispatch: for every case the gates launch and the candidate launch of the cell — with the flags api.hip: gru_cell sets: the second output
    where dispatch.hip: pregate holds, otherwise reset-gate-while-staging on the candidate — land on the kernel family and the tile-table row
    the case's family names (util.tiled_plan / util.wino_plan: the dispatch's own host arithmetic, no GPU).  A retuned threshold fails here
    ("the case no longer exercises what it was chosen for") instead of quietly shrinking what tests/test_gpu_beverse_cells.py covers;
  * every family, and every line of the regime table of the cases, keeps at least one case;
  * sensitivity: each deliberately wrong float64 cell (beverse_cell_util.WRONG) moves a case's output by at least 100 x the case's
    tolerance, and at least a quarter of the reference's update-gate and of its reset-gate values lie in (0.1, 0.9): gates that
    saturate or a tiny state would let a wrong kernel pass;
  * the tolerance constants are the measured table's: 8 x max e32 (+ 2e-5 for the Winograd forms), under 1e-4, and the float32
    reference itself is inside them."""
import os
import re

import pytest

import beverse_cell_util as U
from util import ROOT, maxabs

_IDS = [c["name"] for c in U.CASES]
_NO_LONGER = "the case no longer exercises what it was chosen for"


def _rows():
    src = open(os.path.join(ROOT, "streamingflow_amd", "csrc", "sf_launch.h")).read()
    enum = re.search(r"enum TileId \{(.*?)TILE_COUNT", src, re.S).group(1)
    return [n.strip() for n in enum.split(",") if n.strip()]


@pytest.mark.parametrize("case", U.CASES, ids=_IDS)
def test_case_lands_on_its_family(case):
    rows, p, P, fam = _rows(), U.planned(case), U.pixels(case), case["family"]
    what = (_NO_LONGER, case["name"], fam, p)
    gates, cand = p["gates"], p["cand"]
    pregated_families = ("sp_pregated", "sp_wino", "dma32", "dma64", "dma64_narrow", "wino", "wino_refused")
    assert U.pregated(case) == (fam in pregated_families), what
    if fam in ("sp_pregated", "sp_wino"):
        assert P < U.SP_MAX_P and gates["family"] == 2 and cand["family"] == 2, what
        # the Winograd form of that kernel: the gates launch at least (a 32-channel candidate is half a 64-row tile and keeps the direct form)
        assert U.sp_wino_shape(case, 2 * case["C"]) == (fam == "sp_wino"), what
        assert fam == "sp_wino" or not U.sp_wino_shape(case, case["C"]), what
        if fam == "sp_pregated":
            assert case["n"] > 1 or case["h"] % 2 or case["w"] % 2, what
    elif fam == "wino":
        assert P >= U.WINO_MIN_P and gates["family"] == 1 and cand["family"] == 1, what
        assert p["wino_gates"]["takes"] and p["wino_cand"]["takes"], what
    else:
        assert gates["family"] == 0 and cand["family"] == 0, what
        assert (rows[gates["row"]], rows[cand["row"]]) == U.FAMILIES[fam][1], what
        assert (rows[gates["runs"]], rows[cand["runs"]]) == U.FAMILIES[fam][1], what
        assert not p["wino_gates"]["takes"] and not p["wino_cand"]["takes"], what
        lo, hi = {"direct_gate": (0, U.SP_MAX_P), "staged16_gate": (0, U.SP_MAX_P), "dma32": (U.SP_MAX_P, U.LARGE_P),
                  "direct_gate_mid": (U.SP_MAX_P, U.LARGE_P), "dma64": (U.LARGE_P, U.WINO_MIN_P), "dma64_narrow": (U.LARGE_P, U.WINO_MIN_P),
                  "staged64_gate": (U.LARGE_P, U.WINO_MIN_P), "wino_refused": (U.WINO_MIN_P, 1 << 30)}[fam]
        assert lo <= P < hi, what
        if fam == "direct_gate" or fam == "direct_gate_mid":
            assert case["Cx"] % 8 == 0 and case["C"] % 8 == 0, what
        if fam == "staged16_gate":
            assert case["Cx"] % 8 or case["C"] % 8, what
        if fam == "wino_refused":      # everything but the geometry would have let the Winograd kernel take it
            assert case["w"] < 32 and U.planned(dict(case, w=32))["wino_gates"]["takes"], what
    # the kernel names the GPU test will ask the profiler for
    if p["names"] is None:
        assert U.kernel_prefix(case) == "conv_wino<", what
    else:
        assert len(p["names"]) == 2 and all(k.startswith(U.kernel_prefix(case)) for k in p["names"]), what


def test_every_regime_keeps_a_case():
    by = lambda **kw: [c for c in U.CASES if all(c[k] == v for k, v in kw.items())]
    assert {c["family"] for c in U.CASES} == set(U.FAMILIES), set(U.FAMILIES) - {c["family"] for c in U.CASES}
    # the asymmetric callers: x and state of different widths in every family
    assert all(any(c["Cx"] != c["C"] for c in by(family=f)) or f == "dma64_narrow" for f in U.FAMILIES)
    assert any(c["n"] > 1 for c in by(family="sp_pregated")) and any(c["n"] == 1 and (c["h"] % 2 or c["w"] % 2) for c in by(family="sp_pregated"))
    assert by(family="sp_wino", kind="cell", Cx=288, C=256)                                       # BEVerse's own head width
    assert any(c["Cx"] % 32 and c["Cx"] % 16 == 0 and c["C"] % 32 == 0 for c in by(family="staged64_gate"))      # % 16, not % 32
    assert any((c["h"] + 1) // 2 % 4 for c in by(family="wino")) and any(c["n"] > 1 for c in by(family="wino"))      # tile rows over a multiple of four
    # gru_bias_init on a cell and on a SpatialGRU, both signs
    assert any(c["gru_bias_init"] > 0 for c in by(kind="cell")) and any(c["gru_bias_init"] < 0 for c in by(kind="cell"))
    assert any(c["gru_bias_init"] > 0 for c in by(kind="spatial_gru")) and any(c["gru_bias_init"] < 0 for c in by(kind="spatial_gru"))
    # SpatialGRU without decoder: T > 1, each shape with state=None and with a given state, one of them at P >= 8192
    grus = by(kind="spatial_gru")
    assert grus and all(c["T"] > 1 for c in grus)
    shapes = {(c["Cx"], c["C"], c["n"], c["h"], c["w"], c["T"]) for c in grus}
    assert len(shapes) >= 3 and any(s[2] * s[3] * s[4] >= U.LARGE_P for s in shapes)
    for s in shapes:
        assert {c["given"] for c in grus if (c["Cx"], c["C"], c["n"], c["h"], c["w"], c["T"]) == s} == {True, False}, s


def test_tolerance_is_the_measured_one():
    assert set(U.E32) == set(_IDS)
    assert U.E32_MAX == max(U.E32.values()) and U.TOL_DIRECT == 8 * U.E32_MAX and U.TOL_WINO == U.TOL_DIRECT + 2e-5
    assert 0 < U.TOL_DIRECT < U.TOL_WINO <= U.TOL_CAP == 1e-4
    for c in U.CASES:
        assert U.tolerance(c) == (U.TOL_WINO if c["family"] in ("sp_wino", "wino") else U.TOL_DIRECT)
        assert "%s %.3e" % (c["name"], U.E32[c["name"]]) in U.__doc__      # the docstring's table is the dict
    assert "max e32 = %.3e  ->  TOL_DIRECT = %.3e, TOL_WINO = %.3e" % (U.E32_MAX, U.TOL_DIRECT, U.TOL_WINO) in U.__doc__


@pytest.mark.parametrize("case", U.CASES, ids=_IDS)
def test_float32_reference_is_inside_the_bound(case):
    e32 = maxabs(U.reference32(case), U.reference(case))
    print(case["name"], "e32 now %.3e recorded %.3e bound %.3e" % (e32, U.E32[case["name"]], U.TOL_DIRECT))
    assert e32 <= U.TOL_DIRECT


@pytest.mark.parametrize("case", U.CASES, ids=_IDS)
def test_gates_are_spread(case):
    assert maxabs(U.traced_reference(case), U.reference(case)) <= 1e-13      # the step-by-step cell the wrong variants are made from IS the reference
    for name, g in zip(("update", "reset"), U.gates(case)):
        frac = float(((g > 0.1) & (g < 0.9)).double().mean())
        print(case["name"], name, "gate values in (0.1, 0.9): %.3f" % frac)
        assert frac >= 0.25, (case["name"], name, frac)


@pytest.mark.parametrize("r", U.ROLLOUTS, ids=lambda r: r["name"])
def test_rollout_inputs_are_fit(r):
    """the rollouts of test_gpu_beverse_cells.py: the first step's flow is at least a pixel and samples beyond all four image edges, the
    rollout moves by less than 1e-4 under a 1e-5 input perturbation (so the 1e-3 bar is about the kernels), and the first cell — the
    asymmetric GRUCell(C + L, C) — is planned onto the family the rollout is there for"""
    mag, sides = U.first_flow(r)
    moved = U.perturbation_movement(r)
    print(r["name"], "max |flow| %.2f px, samples outside %s, moves by %.3e under a 1e-5 perturbation" % (mag, sides, moved))
    assert mag >= 1.0 and all(sides.values()), (mag, sides)
    assert moved <= 1e-4, moved
    p = U.planned(dict(Cx=r["C"] + r["L"], C=r["C"], n=r["n"], h=r["h"], w=r["w"]))
    assert (r["prefix"] == "conv_wino<") == (p["names"] is None), (_NO_LONGER, r["name"], p)
    assert p["names"] is None or all(k.startswith(r["prefix"]) for k in p["names"]), (_NO_LONGER, r["name"], p)


@pytest.mark.parametrize("wrong", U.WRONG)
@pytest.mark.parametrize("case", U.CASES, ids=_IDS)
def test_wrong_cell_is_caught(case, wrong):
    if wrong == "bias_dropped" and case["gru_bias_init"] == 0.0:
        assert maxabs(U.wrong_reference(case, wrong), U.reference(case)) <= 1e-13      # nothing to drop: the variant is the reference
        return
    moved = maxabs(U.wrong_reference(case, wrong), U.reference(case))
    print(case["name"], wrong, "moves the output by %.3e = %.0f x the tolerance" % (moved, moved / U.tolerance(case)))
    assert moved >= 100 * U.tolerance(case), (case["name"], wrong, moved)
